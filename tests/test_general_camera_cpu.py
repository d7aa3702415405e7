"""CPU checks that pin the float64 references of the depth, antialias and pose tests at general cameras
(tests/camera_cases.py) before any kernel is compared with them there.  Nothing here needs a GPU.

The bodies are those of test_pose_cpu.py, test_antialias_cpu.py and test_gpu_depth.py, called with another camera; the
bounds are theirs.  The controls at the end mutate a reference in a way that swaps W and W^T in one place: each must
FAIL its check wherever the two differ and PASS at the reference test camera, which is why the identity-camera suite
could not see such a mistake."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import camera_cases as CC
from tests import pose_ref64 as P
from tests import test_antialias_cpu as TAC
from tests import test_gpu_depth as TD
from tests import test_pose_cpu as TPC

WITH_REFERENCE = (CC.REFERENCE,) + CC.ALL


def _packed(name, w, h, n):
    from brush_amd.render import pack_uniforms

    return pack_uniforms(CC.camera(name, w, h), (w, h), 0, n)


def _cloud_for(name, cloud, w, h):
    """Co-moved in front of the camera, except for `free`, which looks at the cloud where it lies."""
    return cloud if name in (CC.REFERENCE, "free") else CC.co_moved(cloud, w, h, name)


# ---------------------------------------------------------------------------- 1. uniforms
@pytest.mark.parametrize("name", WITH_REFERENCE)
def test_pack_uniforms_agrees_with_the_oracle(name):
    """pack_uniforms(Camera) and oracle.make_uniforms agree TO THE BIT at every camera of the table: the same f32
    position and quaternion, the same float64 inverse rounded once; and both hold camera_cases.matrix64 column-major."""
    w, h = 203, 117
    a = CC.camera_args(name, w, h)
    u = _packed(name, w, h, 7)
    o = O.make_uniforms(a["position"], a["rotation_xyzw"], a["fov_x"], a["fov_y"], a["center_uv"], (w, h), 0)
    for field in ("viewmat", "focal", "pixel_center"):
        got = np.array(list(getattr(u, field)), np.float32)
        assert got.tobytes() == np.asarray(o[field], np.float32).tobytes(), (name, field, got, o[field])
    M = CC.matrix64(name, w, h)
    assert np.array_equal(np.array(list(u.viewmat), np.float64).reshape(4, 4).T, M)
    W = M[:3, :3]
    assert np.abs(W @ W.T - np.eye(3)).max() <= 4 * 2.0 ** -24 and np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])
    assert CC.is_symmetric(name) == (name == CC.REFERENCE)
    if name in ("general", "free"):
        assert u.focal[0] != u.focal[1] and tuple(u.pixel_center) != (0.5 * w, 0.5 * h)


def test_co_moved_keeps_camera_space():
    """W_cam (G m) + t_cam = W_ref m + t_ref to the f32 rounding of the moved means, and R(G q) = G_R R(q)."""
    from tests import aa_ref64 as A

    w, h = TPC.FUNCTIONAL_SIZE
    cloud = TPC.functional_cloud()
    m = cloud["means"].astype(np.float64)
    Mr = CC.matrix64(CC.REFERENCE, w, h)
    want = m @ Mr[:3, :3].T + Mr[:3, 3]
    q = cloud["quats"].astype(np.float64)
    for name in CC.CO_MOVED:
        moved = CC.co_moved(cloud, w, h, name)
        Mc = CC.matrix64(name, w, h)
        got = moved["means"].astype(np.float64) @ Mc[:3, :3].T + Mc[:3, 3]
        scale = np.abs(moved["means"]).max() + np.abs(Mc[:3, 3]).max()
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * scale, (name, np.abs(got - want).max())
        qn = np.linalg.norm(q, axis=1, keepdims=True)
        Rc = Mc[:3, :3] @ A.rotmat(moved["quats"].astype(np.float64) / qn)
        assert np.abs(Rc - Mr[:3, :3] @ A.rotmat(q / qn)).max() <= 1e-6, name


# ---------------------------------------------------------------------------- 2. pose restatement
@pytest.mark.parametrize("with_comp", [False, True])
@pytest.mark.parametrize("name", CC.ALL)
def test_restatement_matches_central_differences(name, with_comp):
    """test_pose_cpu.py's check, bound 1e-7, at every camera; _functional_case asserts >= 64 usable splats."""
    w, h = TPC.FUNCTIONAL_SIZE
    cloud = _cloud_for(name, TPC.functional_cloud(), w, h)
    TPC.check_restatement(with_comp, _packed(name, w, h, cloud["means"].shape[0]), cloud)


# ---------------------------------------------------------------------------- 3. the whole chain on the oracle
def _smooth_at(name):
    """test_pose_cpu's _smooth_scene co-moved in front of camera `name` (its own lens as the base)."""
    cloud, u, w, h = TPC._smooth_scene()
    if name == CC.REFERENCE:
        return cloud, u, w, h
    M0 = np.asarray(u["viewmat"], np.float64).reshape(4, 4).T
    return (CC.co_moved(cloud, w, h, name, m_ref=M0), CC.oracle_uniforms(name, w, h, 0, base=TD.SMOOTH_CAMERA), w, h)


@pytest.mark.parametrize("name", CC.CO_MOVED)
def test_whole_chain_against_oracle_finite_differences(name):
    """test_pose_cpu.py's check with its allowance and its "resolves the derivative" assertion."""
    TPC.check_whole_chain(*_smooth_at(name))


# ---------------------------------------------------------------------------- 4. the depth-gradient reference
def check_depth_gradient_reference(name, column=False):
    """d <D, r> / d means along a random direction on the oracle: central differences of the depth-as-colour twin's red
    channel (the twin rebuilt at either side: its colour is z) against the twin backward's v_means plus v_z times row 2
    of W, which is what test_gpu_depth.py adds by hand.  Margin of test_central_difference_wrt_means: 2e-3 relative +
    1e-3, step 1e-2.  `column`: column 2 in place of row 2."""
    cloud, u, w, h = _smooth_at(name)
    un = P.uniforms_ns(u)
    rng = np.random.default_rng(3)
    r = rng.uniform(0.0, 1.0, (h, w))
    d = rng.normal(size=cloud["means"].shape)

    def twin_at(means):
        tw, _ = TD._twin(dict(cloud, means=np.asarray(means, np.float32)), un)
        return tw

    def D(means):
        tw = twin_at(means)
        img, aux = O.render_forward(u, tw["means"], tw["log_scales"], tw["quats"], tw["sh"], tw["raw_opac"])
        return tw, img, aux

    tw, img, aux = D(cloud["means"])
    assert int(aux["num_visible"][0]) == cloud["means"].shape[0]
    assert float(img[..., 3].min()) > 0.05 and float(img[..., 3].max()) < 0.99
    vt = np.zeros((h, w, 4), np.float32)
    vt[..., 0] = r
    g = O.render_backward(u, aux, tw["means"], tw["log_scales"], tw["quats"], tw["raw_opac"], img, vt)
    v_z = g["v_sh"][:, 0, 0].astype(np.float64) / float(TD.C0)
    v_means = g["v_means"].astype(np.float64) + v_z[:, None] * TD._z_row(un, column)[None, :]
    analytic = float((v_means * d).sum())
    eps = 1e-2
    m0 = cloud["means"].astype(np.float64)
    fd = (float((D(m0 + eps * d)[1][..., 0].astype(np.float64) * r).sum())
          - float((D(m0 - eps * d)[1][..., 0].astype(np.float64) * r).sum())) / (2 * eps)
    print(f"[{name} column={column}] analytic {analytic:+.6e} fd {fd:+.6e} |a - fd| / |fd| "
          f"{abs(analytic - fd) / abs(fd):.3e}; the depth term is {float((v_z[:, None] * TD._z_row(un)[None, :] * d).sum()):+.3e}")
    assert abs(analytic - fd) <= 2e-3 * abs(fd) + 1e-3, (name, analytic, fd)


@pytest.mark.parametrize("name", (CC.REFERENCE,) + CC.CO_MOVED)
def test_depth_gradient_reference_matches_central_differences(name):
    check_depth_gradient_reference(name)


# ---------------------------------------------------------------------------- 5. the antialias reference
@pytest.mark.parametrize("name", CC.ALL)
def test_comp_vjp_matches_central_differences(name):
    w, h = TAC.CASES_SIZE
    cloud = _cloud_for(name, TAC.cases_cloud(), w, h)
    TAC.check_comp_vjp(_packed(name, w, h, cloud["means"].shape[0]), cloud)


# ---------------------------------------------------------------------------- 6. mutation controls
def _rows_differ(name):
    W = CC.matrix64(name)[:3, :3]
    return bool(np.abs(W[2, :] - W[:, 2]).max() > 1e-6)


@pytest.mark.parametrize("name", (CC.REFERENCE,) + CC.CO_MOVED)
def test_control_depth_term_with_column_2(name):
    """Column 2 of W in place of row 2 fails the depth-gradient check wherever the two differ, and passes where they
    are the same vector: at the reference camera, and under roll_z, whose W is not symmetric but keeps row 2 and
    column 2 at (0, 0, 1) (the case that tells an x/y mix-up from a z-row mistake)."""
    if _rows_differ(name):
        with pytest.raises(AssertionError):
            check_depth_gradient_reference(name, column=True)
    else:
        assert name in (CC.REFERENCE, "roll_z")
        check_depth_gradient_reference(name, column=True)


@pytest.mark.parametrize("with_comp", [False, True])
@pytest.mark.parametrize("mutate", P.MUTATIONS)
@pytest.mark.parametrize("name", WITH_REFERENCE)
def test_control_pose_restatement_with_w_transposed(name, mutate, with_comp):
    """Each of pose_ref64.MUTATIONS fails the restatement's central-difference check at every camera whose W is not
    symmetric and passes it at the reference test camera."""
    w, h = TPC.FUNCTIONAL_SIZE
    cloud = _cloud_for(name, TPC.functional_cloud(), w, h)
    u = _packed(name, w, h, cloud["means"].shape[0])
    if CC.is_symmetric(name):
        TPC.check_restatement(with_comp, u, cloud, mutate=mutate)
    else:
        with pytest.raises(AssertionError):
            TPC.check_restatement(with_comp, u, cloud, mutate=mutate)


@pytest.mark.parametrize("mutate", P.MUTATIONS)
def test_control_whole_chain_with_w_transposed(mutate):
    """The same mutations against the oracle's own finite differences: caught under `general`, unseen at the reference
    camera."""
    TPC.check_whole_chain(*_smooth_at(CC.REFERENCE), mutate=mutate)
    with pytest.raises(AssertionError):
        TPC.check_whole_chain(*_smooth_at("general"), mutate=mutate)


# ---------------------------------------------------------------------------- 7. scene conditions of the GPU tests
@pytest.mark.parametrize("kind,name", CC.GPU_SCENES)
def test_gpu_scene_conditions_hold_on_the_oracle(kind, name):
    """camera_cases.scene_at asserts them; here they are checked without a GPU, and the counts are printed."""
    for normalised in (False, True):
        _, _, _, facts = CC.scene_at(kind, name, normalised)
        print(kind, name, normalised, facts)
        assert facts["visible"] > 0 and facts["flip_risk"] <= CC.MAX_FLIP_FRACTION


# ---------------------------------------------------------------------------- 8. rehearsal of the GPU pose fit
def fit_problem_at(name):
    """(cloud, oracle uniforms, w, h) of pose_ref64.fit_problem co-moved in front of camera `name`."""
    w, h = P.FIT_W, P.FIT_H
    return CC.co_moved(P.fit_problem(), w, h, name), CC.oracle_uniforms(name, w, h, 0), w, h


def test_pose_fit_rehearsal_on_the_oracle_under_general():
    """test_pose_cpu.py's rehearsal with the fit problem co-moved with `general`: the same FIT_STEPS, FIT_LR and
    FIT_DELTA, the same end condition.  tests/test_gpu_general_camera.py repeats it on the GPU."""
    TPC.check_pose_fit_rehearsal(*fit_problem_at("general"))
