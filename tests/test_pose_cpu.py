"""CPU checks of the camera-pose gradient and the pose optimiser (brush_render_backward_pose, brush_amd/pose.py): the
float64 restatement against central differences, the whole chain on the CPU oracle, se3_exp, PoseTable's Adam, the new
entry points' argument checks and the CLI flags.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import aa_ref64 as A
from tests import helpers as H
from tests import pose_ref64 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


def _uniforms(w, h, n):
    import brush_amd
    from brush_amd.render import pack_uniforms

    c = H.reference_test_camera(w, h)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    return pack_uniforms(cam, (w, h), 0, n)


# ---------------------------------------------------------------------------- 1. restatement vs central differences
FUNCTIONAL_SIZE = (160, 120)


def functional_cloud():
    return H.synthetic_cloud(4000, 0, seed=11, mean_mult=1.0)


def _functional_case(u=None, cloud=None):
    """`u`: packed uniforms of a FUNCTIONAL_SIZE frame (default: the reference test camera's); `cloud`: the cloud the
    splats are taken from (default: functional_cloud())."""
    cloud = functional_cloud() if cloud is None else cloud
    u = P.uniforms_ns(_uniforms(*FUNCTIONAL_SIZE, cloud["means"].shape[0]) if u is None else u)
    means = cloud["means"].astype(np.float64)
    ls = cloud["log_scales"].astype(np.float64)
    q = cloud["quats"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    W, t = P.view_of(u)
    z = (means @ W.T + t)[:, 2]
    comp = A.comp64(u, means, ls, q)
    ok = (z > 0.5) & ~A.clamp_active(u, means) & (comp > 0.02) & (comp < 0.98)
    idx = np.nonzero(ok)[0][:96]
    assert idx.size >= 64, idx.size
    return u, means[idx], ls[idx], q[idx]


@pytest.mark.parametrize("with_comp", [False, True])
def test_restatement_matches_central_differences(with_comp):
    """F([W | t]) = sum_i a_i . xy_i + <B_i, cov2d_i> + c_i z_i (+ d_i g(comp_i)) in float64 over a random cloud with the
    frustum clamp inactive, differentiated entry by entry of [W | t] (the formulas hold for any 3x3 W).  xy is taken
    with the projection's own 1 / (z + 1e-6); g(c) = c - 1e-6 ln(c + 1e-6) is the function whose derivative is the
    backward's comp / (comp + 1e-6), so the functional's exact gradient is the backward's formula.  Central differences
    at h = 1e-5 of O(1..10) entries: truncation ~1e-10 f''', rounding ~1e-16 |F| / 1e-5: the bound asked is 1e-7
    relative to the largest entry."""
    check_restatement(with_comp)


def check_restatement(with_comp, u=None, cloud=None, mutate=None):
    """The body of test_restatement_matches_central_differences at the camera of the packed uniforms `u`, on splats of
    `cloud`; `mutate` names a deliberate mistake of pose_ref64.pose_grad64 (its MUTATIONS), for the controls."""
    u, m, ls, q = _functional_case(u, cloud)
    n = m.shape[0]
    rng = np.random.default_rng(5)
    a = rng.normal(size=(n, 2))
    B = rng.normal(size=(n, 2, 2)) * 1e-2
    B = B + np.transpose(B, (0, 2, 1))
    c = rng.normal(size=n)
    d = rng.uniform(0.5, 1.5, n) if with_comp else None
    W0, t0 = P.view_of(u)

    def F(W, t):
        uu = P.with_view(u, W, t)
        p = m @ W.T + t
        rw = 1.0 / (p[:, 2] + 1e-6)
        xy = uu.focal[None, :] * p[:, :2] * rw[:, None] + uu.pixel_center[None, :]
        cov, blurred = A.cov2d64(uu, m, ls, q)
        val = (a * xy).sum() + (B * cov).sum() + (c * p[:, 2]).sum()
        if d is not None:
            comp = A.comp_from(cov, blurred)
            val += (d * (comp - 1e-6 * np.log(comp + 1e-6))).sum()
        return val

    # v_conic that makes the chain's v_cov equal B: v_cov = -conic G conic  <=>  G = -S B S, S the blurred covariance
    _, S = A.cov2d64(u, m, ls, q)
    G = -(S @ B @ S)
    v_conic = np.stack([G[:, 0, 0], 2.0 * G[:, 0, 1], G[:, 1, 1]], -1)
    got, mag = P.pose_grad64(u, m, ls, q, a, v_conic, v_z=c, v_comp=d, mutate=mutate)
    fd = np.zeros((3, 4))
    h = 1e-5
    for r in range(3):
        for k in range(4):
            Wp, Wm, tp, tm = W0.copy(), W0.copy(), t0.copy(), t0.copy()
            if k < 3:
                Wp[r, k] += h
                Wm[r, k] -= h
            else:
                tp[r] += h
                tm[r] -= h
            fd[r, k] = (F(Wp, tp) - F(Wm, tm)) / (2 * h)
    rel = np.abs(got - fd).max() / np.abs(fd).max()
    print(f"comp={with_comp}: max|analytic - fd| / max|fd| = {rel:.3e}; per entry / mag: "
          f"{(np.abs(got - fd) / mag).max():.3e}")
    assert (mag >= np.abs(got) * (1 - 1e-12)).all()
    assert rel <= 1e-7, rel
    return rel


# ---------------------------------------------------------------------------- 2. the whole chain on the CPU oracle
CHAIN_H = 1.6e-2  # twist step of the central differences (radians / world units); see the test's docstring


def _oracle_scene():
    cloud = P.fit_problem()
    w, h = P.FIT_W, P.FIT_H
    u = O.make_uniforms(**{k: v for k, v in H.reference_test_camera(w, h).items()}, img_size=(w, h), sh_degree=0)
    return cloud, u, w, h


def _smooth_scene():
    """Six broad splats in front of an identity camera on a 32 x 32 frame: every splat's alpha stays above 1/255 on the
    whole frame (and over the steps of the differences) and the transmittance far above its stop, so the image is a
    smooth function of the pose: no threshold is crossed between the two sides of a central difference."""
    w = h = 32
    u = O.make_uniforms([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], 0.5, 0.5, (0.5, 0.5), (w, h), 0)
    means = np.float32([[0.2, -0.1, 5.0], [-0.3, 0.2, 6.5], [0.1, 0.3, 8.0], [-0.2, -0.25, 4.5], [0.35, 0.1, 7.0],
                        [-0.1, -0.3, 5.5]])
    log_scales = np.log(np.float32([[2.0, 1.6, 0.7], [1.8, 2.2, 1.0], [2.5, 2.0, 1.5], [1.7, 1.9, 0.5],
                                    [2.1, 2.4, 0.9], [1.9, 1.7, 1.2]]))
    q = np.float64([[1.0, 0.1, 0.0, 0.05], [0.9, 0.0, 0.2, 0.0], [1.0, -0.1, 0.1, 0.1], [1.0, 0.0, 0.0, -0.2],
                    [0.95, 0.1, -0.1, 0.0], [1.0, 0.05, 0.15, 0.1]])
    quats = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sh = np.float32([[[0.9, -0.4, 0.2]], [[-0.6, 0.8, 0.1]], [[0.3, 0.3, -0.9]], [[-0.2, -0.7, 0.6]],
                     [[0.7, 0.1, 0.5]], [[-0.8, 0.5, -0.3]]])
    raw_opac = np.float32([-1.0, -1.5, -0.7, -2.0, -1.2, -1.6])
    return dict(means=means, log_scales=log_scales, quats=quats, sh=sh, raw_opac=raw_opac), u, w, h


def _with_matrix(u, M):
    uu = dict(u)
    uu["viewmat"] = np.ascontiguousarray(np.asarray(M, np.float32).T).reshape(16)
    return uu


def _oracle_image(u, cloud):
    return O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"])


def oracle_pose_grad(u, cloud, v_out_fn, mutate=None):
    """(image, v_viewmat [3,4], mag) of <image, v_out> on the CPU: oracle forward / backward, then pose_grad64 on the
    backward's compact sums.  v_out_fn(image) -> v_out."""
    img, aux = _oracle_image(u, cloud)
    v_out = np.ascontiguousarray(v_out_fn(img), np.float32)
    g = O.render_backward(u, aux, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["raw_opac"], img, v_out)
    V = int(aux["num_visible"][0])
    gids = aux["global_from_compact_gid"][:V]
    got, mag = P.pose_grad64(P.uniforms_ns(u), cloud["means"], cloud["log_scales"], cloud["quats"],
                             g["v_xy_local"][:V], g["v_conics"][:V], gids=gids, mutate=mutate)
    return img, got, mag


def test_whole_chain_against_oracle_finite_differences():
    """d <image, v_out> / d twist along the six twist axes, SH degree 0, clamp inactive: central differences of the
    oracle's f32 forward at steps h and 2h against pose_grad64 on the oracle backward's (v_xy_local, v_conics).  The
    analytic side is contracted with the very difference of the two f32 matrices the forward was given, so the rounding
    of the matrices is not part of the comparison.  Asked: |analytic - fd(h)| <= 4 |fd(h) - fd(2h)| + floor; the
    truncation error of fd(h) is a third of |fd(h) - fd(2h)| for a smooth function, so 4 leaves room for the
    piecewise-constant decisions (alpha threshold, tile lists) both differences cross.  floor: the f32 image carries
    rounding errors of at most ~64 eps32 per value (aa_ref64.K_COV counts the projection chain alone), two images per
    difference: 2 * 64 eps32 sum|image . v_out| / (2h).  h = 1.6e-2 was chosen on the CPU (POSE_CHAIN_SCAN=1 prints the
    scan): there |analytic - fd| follows h^2 at a twelfth of the allowance and the floor is 3 % of the smallest of
    the six derivatives; at 1e-3 the floor would be half of it.  The scene (_smooth_scene) crosses no threshold."""
    check_whole_chain(*_smooth_scene())


def check_whole_chain(cloud, u, w, h, mutate=None):
    """The body of test_whole_chain_against_oracle_finite_differences on a scene and the oracle uniforms of its
    camera."""
    M0 = np.asarray(u["viewmat"], np.float64).reshape(4, 4).T
    img_chk, aux_chk = _oracle_image(u, cloud)
    assert int(aux_chk["num_visible"][0]) == cloud["means"].shape[0]
    assert float(img_chk[..., 3].min()) > 0.05 and float(img_chk[..., 3].max()) < 0.99
    assert not A.clamp_active(P.uniforms_ns(u), cloud["means"]).any()
    # a smooth upstream gradient (a random quadratic of the pixel position per channel): the derivative is a coherent
    # sum over the frame, large against the rounding floor, which counts every pixel's error with the same sign
    rng = np.random.default_rng(9)
    yy, xx = np.meshgrid((np.arange(h) - h / 2) / (h / 2), (np.arange(w) - w / 2) / (w / 2), indexing="ij")
    basis = np.stack([np.ones_like(xx), xx, yy, xx * yy, xx * xx, yy * yy], -1)
    v_out = (basis @ rng.uniform(-0.5, 0.5, (6, 4))).astype(np.float32)
    img0, g34, mag = oracle_pose_grad(u, cloud, lambda im: v_out, mutate=mutate)
    floor_unit = 64 * EPS32 * float(np.abs(img0.astype(np.float64) * v_out).sum())

    def fd(j, step):
        e = np.zeros(6)
        e[j] = step
        Mp = (P.expm_series(P.twist_matrix(e)) @ M0).astype(np.float32)
        Mm = (P.expm_series(P.twist_matrix(-e)) @ M0).astype(np.float32)
        Fp = float((_oracle_image(_with_matrix(u, Mp), cloud)[0].astype(np.float64) * v_out).sum())
        Fm = float((_oracle_image(_with_matrix(u, Mm), cloud)[0].astype(np.float64) * v_out).sum())
        dM = Mp.astype(np.float64) - Mm.astype(np.float64)
        return (Fp - Fm) / (2 * step), float((g34 * dM[:3]).sum()) / (2 * step)

    for j in range(6):
        if os.environ.get("POSE_CHAIN_SCAN"):  # measurement aid: the figures at other steps
            for hh in (1e-3, 4e-3, 8e-3, 1.6e-2, 3.2e-2):
                x1, y1 = fd(j, hh)
                x2, _ = fd(j, 2 * hh)
                print(f"  h {hh:g}: analytic {y1:+.6e} fd {x1:+.6e} |a - fd| {abs(y1 - x1):.2e} 4|d| "
                      f"{4 * abs(x1 - x2):.2e} floor {2 * floor_unit / (2 * hh):.2e}")
        f1, a1 = fd(j, CHAIN_H)
        f2, _ = fd(j, 2 * CHAIN_H)
        allow = 4 * abs(f1 - f2) + 2 * floor_unit / (2 * CHAIN_H)
        print(f"twist {j}: analytic {a1:+.6e} fd(h) {f1:+.6e} fd(2h) {f2:+.6e} |a - fd| {abs(a1 - f1):.3e} "
              f"allowed {allow:.3e}")
        assert abs(a1 - f1) <= allow, (j, a1, f1, f2, allow)
        assert abs(a1) > 10 * allow, (j, a1, allow)  # the check resolves the derivative


# ---------------------------------------------------------------------------- 3. se3_exp
@pytest.mark.parametrize("theta", [0.0, 1e-8, 1e-4, 1.0, 3.0])
def test_se3_exp_is_the_matrix_exponential(theta):
    import torch

    from brush_amd.pose import apply_delta, se3_exp

    axis = np.array([0.3, -0.5, 0.8])
    axis = axis / np.linalg.norm(axis)
    delta = np.concatenate([theta * axis, [0.4, -0.7, 1.1]])
    M = se3_exp(torch.tensor(delta)).numpy()
    assert M.dtype == np.float64 and M.shape == (4, 4)
    if theta == 0.0:
        assert np.array_equal(M[:3, :3], np.eye(3)) and np.array_equal(M[:3, 3], delta[3:])
        assert np.array_equal(se3_exp(torch.zeros(6)).numpy(), np.eye(4))
    R = M[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4e-16 and abs(np.linalg.det(R) - 1.0) <= 4e-16
    assert np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])
    assert np.abs(M - P.expm_series(P.twist_matrix(delta))).max() <= 1e-14
    base = np.eye(4)
    base[:3, 3] = [1.0, 2.0, 3.0]
    assert np.allclose(apply_delta(torch.tensor(base), torch.tensor(delta)).numpy(), M @ base, rtol=0, atol=1e-15)


@pytest.mark.parametrize("theta", [0.0, 1e-4, 0.0999, 0.1001, 1.0, 3.0])
def test_se3_exp_gradient_matches_central_differences(theta):
    import torch

    from brush_amd.pose import se3_exp

    axis = np.array([-0.6, 0.2, 0.5])
    axis = axis / np.linalg.norm(axis)
    delta = np.concatenate([theta * axis, [0.4, -0.7, 1.1]])
    Wt = np.random.default_rng(2).normal(size=(4, 4))
    d = torch.tensor(delta, requires_grad=True)
    (se3_exp(d) * torch.tensor(Wt)).sum().backward()
    got = d.grad.numpy()
    assert np.isfinite(got).all()
    fd = np.zeros(6)
    for j in range(6):
        e = np.zeros(6)
        e[j] = 1e-6
        fd[j] = ((P.expm_series(P.twist_matrix(delta + e)) - P.expm_series(P.twist_matrix(delta - e))) * Wt).sum() / 2e-6
    assert np.abs(got - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max()), (got, fd)


# ---------------------------------------------------------------------------- 4. PoseTable
def test_pose_table_apply_is_adam_in_float64():
    import torch

    from brush_amd.pose import PoseTable, apply_delta

    rng = np.random.default_rng(4)
    lr_rot, lr_trans, reg = 3e-3, 2e-2, 1e-3
    tab = PoseTable(3, lr_rot, lr_trans, reg)
    base = np.eye(4)
    base[:3, :3] = P.expm_series(P.twist_matrix([0.2, -0.1, 0.3, 0, 0, 0]))[:3, :3]
    base[:3, 3] = [0.5, -1.0, 6.0]
    tab.set_base(1, base)
    assert tab.apply(1) is False  # nothing pending
    assert np.array_equal(tab.viewmat(1).numpy(), base.astype(np.float32))
    delta, m1, m2 = np.zeros(6), np.zeros(6), np.zeros(6)
    lr = np.array([lr_rot] * 3 + [lr_trans] * 3)
    for t in range(1, 6):
        g34 = rng.normal(size=(3, 4)).astype(np.float32)
        tab.push(1, g34)
        assert tab.apply(1) is True and tab.apply(1) is False
        # hand-written: chain by central differences of the series exponential, then Adam
        g = np.zeros(6)
        for j in range(6):
            e = np.zeros(6)
            e[j] = 1e-6
            dM = (P.expm_series(P.twist_matrix(delta + e)) - P.expm_series(P.twist_matrix(delta - e))) @ base / 2e-6
            g[j] = (dM[:3] * g34.astype(np.float64)).sum()
        g = g + reg * delta
        m1 = 0.9 * m1 + 0.1 * g
        m2 = 0.999 * m2 + 0.001 * g * g
        delta = delta - lr * (m1 / (1 - 0.9 ** t)) / (np.sqrt(m2 / (1 - 0.999 ** t)) + 1e-15)
        # Adam's first steps are lr * sign-like: a relative gradient error of 1e-9 moves the step by as much
        assert np.abs(tab.delta[1].numpy() - delta).max() <= 1e-7 * lr.max(), (t, tab.delta[1].numpy(), delta)
        want = (P.expm_series(P.twist_matrix(delta)) @ base).astype(np.float32)
        assert np.abs(tab.viewmat(1).numpy() - want).max() <= 1e-6
    assert tab.steps == [0, 5, 0] and not tab.delta[0].any() and not tab.delta[2].any()
    tab.push(0, np.ones(12, np.float32))
    with pytest.raises(ValueError):
        tab.viewmat(2)
    tab.set_base(0, base)
    assert tab.apply_all() == 1 and tab.steps == [1, 5, 0]
    assert len(tab.deltas()) == 3 and len(tab.deltas()[0]) == 6
    # apply_delta is differentiable down to delta
    d = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    apply_delta(torch.tensor(base), d)[:3].sum().backward()
    assert bool(torch.isfinite(d.grad).all()) and bool(d.grad.abs().sum() > 0)


# ---------------------------------------------------------------------------- 5. argument validation, no GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_pose_entry_points_validate_arguments_without_gpu(lib):
    n = C.c_size_t()
    assert lib.brush_pose_grad_workspace_size(1 << 20, None) == -1
    assert lib.brush_pose_grad_workspace_size(0, C.byref(n)) == 0 and n.value >= 96
    assert lib.brush_pose_grad_workspace_size(1, C.byref(n)) == 0 and n.value >= 96
    assert lib.brush_pose_grad_workspace_size(1 << 24, C.byref(n)) == 0 and 96 <= n.value <= (1 << 20)
    big = n.value
    one = C.c_void_p(16)  # a non-null pointer that is never dereferenced: every check below fails before device work
    nulls18 = [None] * 6 + [0] + [None] * 10
    # brush_render_backward_pose(u, aux, means, log_scales, quats, raw_opac, n, out, v_out, compact_depth, v_depth,
    #                            v_means, v_xy, v_scales, v_quats, v_sh, v_opac, ws, ws_bytes, v_viewmat, pose_ws, bytes, s)
    assert lib.brush_render_backward_pose(*nulls18, None, 0, None, one, big, None) == -1   # null v_viewmat
    assert lib.brush_render_backward_pose(*nulls18, None, 0, one, None, big, None) == -1   # null pose workspace
    args = [None] * 6 + [1 << 24] + [None] * 10
    assert lib.brush_render_backward_pose(*args, None, 0, one, one, big - 1, None) == -2   # small pose workspace
    assert lib.brush_render_backward_pose(*nulls18, None, 0, one, one, big, None) == -1    # null uniforms / aux
    # brush_render_backward_adam_pose(u, aux, cfg, means, log_scales, quats_fed, rotation, raw_opac, sh, n, out, v_out,
    #                                 v_xy, m1, m2, next_quats, g2d, counts, ws, ws_bytes, v_viewmat, pose_ws, bytes, s)
    head = [None] * 9 + [0] + [None] * 8
    assert lib.brush_render_backward_adam_pose(*head, None, 0, None, one, big, None) == -1
    assert lib.brush_render_backward_adam_pose(*head, None, 0, one, None, big, None) == -1
    head_big = [None] * 9 + [1 << 24] + [None] * 8
    assert lib.brush_render_backward_adam_pose(*head_big, None, 0, one, one, big - 1, None) == -2
    assert lib.brush_render_backward_adam_pose(*head, None, 0, one, one, big, None) == -1  # null config
    assert lib.brush_status_string(-2) == b"workspace too small"


def test_python_surface_without_gpu():
    import inspect

    import torch

    import brush_amd
    from brush_amd import render as R

    assert "viewmat" in inspect.signature(R.pack_uniforms).parameters
    sig = inspect.signature(brush_amd.render_splats_pose)
    for name in ("viewmat", "deterministic", "antialiased", "depth"):
        assert name in sig.parameters, name
    assert hasattr(brush_amd.Splats, "render_pose")
    for name in ("pose_opt", "lr_pose_rot", "lr_pose_trans", "pose_reg"):
        assert hasattr(brush_amd.TrainConfig(), name), name
    assert brush_amd.TrainConfig().pose_opt is False
    assert "poses" in inspect.signature(brush_amd.SplatTrainer.step).parameters
    # an explicit matrix replaces the camera's, column-major in the uniforms; focal and centre stay the camera's
    c = H.reference_test_camera(64, 48)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    M = np.arange(16, dtype=np.float32).reshape(4, 4)
    u0, u1 = R.pack_uniforms(cam, (64, 48), 0, 5), R.pack_uniforms(cam, (64, 48), 0, 5, viewmat=M)
    assert list(u1.viewmat) == [float(M[r, c]) for c in range(4) for r in range(4)]
    assert list(u1.focal) == list(u0.focal) and list(u1.pixel_center) == list(u0.pixel_center)
    u2 = R.pack_uniforms(cam, (64, 48), 0, 5, viewmat=cam.world_to_local())
    assert list(u2.viewmat) == list(u0.viewmat)
    # the op refuses CPU splats like its neighbours
    z = torch.zeros
    with pytest.raises(AssertionError, match="no CPU path"):
        brush_amd.render_splats_pose(cam, (32, 32), z((4, 3)), None, z((4, 3)), z((4, 4)), z((4, 1, 3)), z((4,)),
                                     torch.eye(4))


def test_cli_flags():
    from brush_amd import train_loop as TL

    p = TL.parser()
    a = p.parse_args(["data"])
    assert a.pose_opt is False and a.export_cameras is None
    a = p.parse_args(["data", "--pose-opt", "--export-cameras", "cams.json"])
    assert a.pose_opt is True and a.export_cameras == "cams.json"
    log = TL.TrainLog(0, np.zeros(0, np.float32))
    js = log.to_json()
    assert js["pose_opt"] is False and js["pose_deltas"] is None


# ---------------------------------------------------------------------------- 6. rehearsal of the GPU pose fit
def test_pose_fit_rehearsal_on_the_oracle():
    """The run tests/test_gpu_pose.py repeats on the GPU: splats fixed, the target is the render at the true pose, the
    start is the perturbed pose (pose_ref64.FIT_*), Adam on the twist through the oracle forward / backward and
    pose_grad64.  It must end below one tenth of its initial rotation and translation error."""
    check_pose_fit_rehearsal(*_oracle_scene())


def check_pose_fit_rehearsal(cloud, u, w, h):
    import torch

    M_true = np.asarray(u["viewmat"], np.float64).reshape(4, 4).T
    target = _oracle_image(u, cloud)[0].astype(np.float64)
    npix = float(w * h)

    class OracleLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, viewmat):
            uu = _with_matrix(u, viewmat.numpy())
            img, g34, _ = oracle_pose_grad(uu, cloud, lambda im: (im.astype(np.float64) - target) / npix)
            g = np.zeros((4, 4), np.float32)
            g[:3] = g34
            ctx.g = torch.from_numpy(g)
            return torch.tensor(0.5 * float(((img.astype(np.float64) - target) ** 2).sum()) / npix)

        @staticmethod
        def backward(ctx, v):
            return ctx.g * v

    first, last, losses = P.fit_pose(OracleLoss.apply, M_true)
    print(f"rotation {first[0]:.4f} -> {last[0]:.5f} rad, translation {first[1]:.4f} -> {last[1]:.5f}; "
          f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert last[0] < 0.1 * first[0] and last[1] < 0.1 * first[1], (first, last)
