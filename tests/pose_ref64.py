"""float64 restatement of the camera-pose gradient (include/brush_hip.h: brush_render_backward_pose).

With p = W mean + t and T = J W, from the per-visible-splat gradients the compositing backward leaves (v_xy, v_conic,
optionally v_z of the accumulated depth and v_comp of the antialiased mode's opacity factor):

    v_p  = project_pix_vjp(v_xy) + v_t(v_J) + (0, 0, v_z)        v_T = 2 v_cov T V
    v_t_view = sum v_p                                           v_W = sum ( v_p mean^T + J^T v_T )

exactly as splat_vjp.hpp chains them: v_cov from v_conic through the inverse of the blurred covariance (plus the comp
term), J at the UNCLAMPED p_view, 1 / (z + 1e-6) in the pixel projection, no gradient through the SH view direction.
The projection pieces are aa_ref64's.  `pose_grad64` also returns, per entry, the sum over splats of the absolute values
of the terms the entry is made of: the scale rounding errors and cancellation are measured against.

Also here, because the CPU rehearsal and the GPU test must run the same problem: the pose-fit scene (`fit_problem`) and
its Adam loop (`fit_pose`)."""
import types

import numpy as np

from tests import aa_ref64 as A


def uniforms_ns(u):
    """BrushUniforms / uniforms_to_numpy dict -> a namespace with float64 numpy fields (viewmat column-major [16])."""
    get = (lambda k: u[k]) if isinstance(u, dict) else (lambda k: getattr(u, k))
    return types.SimpleNamespace(viewmat=np.array(list(get("viewmat")), np.float64),
                                 focal=np.array(list(get("focal")), np.float64),
                                 pixel_center=np.array(list(get("pixel_center")), np.float64),
                                 img_size=np.array(list(get("img_size")), np.float64))


def with_view(u, W, t):
    """A copy of the namespace `u` with the world-to-camera transform [W | t] (any 3x3 W: the formulas do not need a
    rotation)."""
    vm = np.array(u.viewmat, np.float64).copy()
    for r in range(3):
        for c in range(3):
            vm[c * 4 + r] = W[r, c]
        vm[12 + r] = t[r]
    return types.SimpleNamespace(viewmat=vm, focal=u.focal, pixel_center=u.pixel_center, img_size=u.img_size)


def view_of(u):
    W, t, _, _, _ = A._view(u)
    return W, t


# Deliberate mistakes for the controls of tests/test_general_camera_cpu.py: each swaps W and W^T in one place, so it is
# invisible where W is symmetric (the reference test camera's W = I) and wrong everywhere else.
MUTATIONS = ("T=J.W^T",        # the backward's T = J W taken as J W^T
             "v_J=v_T.W",      # the VJP through W of T = J W transposed: v_J = v_T W^T taken as v_T W
             "v_t=W^T.sum")    # the translation gradient taken through W^T: W^T sum v_p, the world-frame sum v_means


def pose_terms64(u, means, log_scales, quats, v_xy, v_conic, v_z=None, v_comp=None, mutate=None):
    """Per splat: (v_p parts [3 x [N,3]]: pixel, Jacobian, depth; J [N,2,3]; v_T [N,2,3]; mean [N,3])."""
    assert mutate is None or mutate in MUTATIONS, mutate
    W, f, pc, img, p, scale, R, M, V = A._parts(u, means, log_scales, quats)
    n = p.shape[0]
    v_xy = np.asarray(v_xy, np.float64).reshape(n, 2)
    v_conic = np.asarray(v_conic, np.float64).reshape(n, 3)
    cov, blurred = A.cov2d64(u, means, log_scales, quats)
    det = blurred[:, 0, 0] * blurred[:, 1, 1] - blurred[:, 0, 1] ** 2
    conic = np.stack([np.stack([blurred[:, 1, 1], -blurred[:, 0, 1]], -1),
                      np.stack([-blurred[:, 1, 0], blurred[:, 0, 0]], -1)], 1) / det[:, None, None]
    G = np.stack([np.stack([v_conic[:, 0], 0.5 * v_conic[:, 1]], -1),
                  np.stack([0.5 * v_conic[:, 1], v_conic[:, 2]], -1)], 1)
    v_cov = -(conic @ G @ conic)  # cov2d_to_conic_vjp
    if v_comp is not None:
        comp = A.comp_from(cov, blurred)
        inv_det = conic[:, 0, 0] * conic[:, 1, 1] - conic[:, 0, 1] ** 2
        v_sqr = np.where(comp > 0, np.asarray(v_comp, np.float64) * 0.5 / (comp + 1e-6), 0.0)
        v_cov = v_cov + v_sqr[:, None, None] * ((1 - comp * comp)[:, None, None] * conic
                                                - A.COV_BLUR * inv_det[:, None, None] * np.eye(2))
    z = p[:, 2]
    rw = 1.0 / (z + 1e-6)
    a0, a1 = f[0] * v_xy[:, 0], f[1] * v_xy[:, 1]
    vpj = np.stack([a0 * rw, a1 * rw, -(a0 * p[:, 0] + a1 * p[:, 1]) * rw * rw], -1)
    J = A._jac(f, p, p[:, 0], p[:, 1])
    T = J @ (W.T if mutate == "T=J.W^T" else W)
    v_T = 2.0 * v_cov @ T @ V
    v_J = v_T @ (W if mutate == "v_J=v_T.W" else W.T)
    rz2, rz3 = 1 / z ** 2, 1 / z ** 3
    v_t = np.stack([-f[0] * rz2 * v_J[:, 0, 2], -f[1] * rz2 * v_J[:, 1, 2],
                    -f[0] * rz2 * v_J[:, 0, 0] + 2 * f[0] * p[:, 0] * rz3 * v_J[:, 0, 2]
                    - f[1] * rz2 * v_J[:, 1, 1] + 2 * f[1] * p[:, 1] * rz3 * v_J[:, 1, 2]], -1)
    vz = np.zeros((n, 3))
    if v_z is not None:
        vz[:, 2] = np.asarray(v_z, np.float64).reshape(n)
    return (vpj, v_t, vz), J, v_T, np.asarray(means, np.float64)


def pose_grad64(u, means, log_scales, quats, v_xy, v_conic, v_z=None, v_comp=None, gids=None, mutate=None):
    """(v_viewmat [3,4], mag [3,4]).  v_xy [V,2], v_conic [V,3], v_z [V], v_comp [V] belong to the visible splats in
    compact order, `gids` [V] maps them to rows of means / log_scales / quats (None: the arrays are already per visible
    splat).  Row r of the result is [d L / d W[r, :] | d L / d t[r]].  `mutate`: one of MUTATIONS, for the controls."""
    if gids is not None:
        gids = np.asarray(gids).astype(np.int64)
        means, log_scales, quats = (np.asarray(a)[gids] for a in (means, log_scales, quats))
    out, mag = np.zeros((3, 4)), np.zeros((3, 4))
    if np.asarray(means).shape[0] == 0:
        return out, mag
    parts, J, v_T, m = pose_terms64(u, means, log_scales, quats, v_xy, v_conic, v_z, v_comp, mutate)
    v_p = parts[0] + parts[1] + parts[2]
    a_p = np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])
    out[:, :3] = np.einsum("na,nb->ab", v_p, m) + np.einsum("nra,nrb->ab", J, v_T)
    mag[:, :3] = np.einsum("na,nb->ab", a_p, np.abs(m)) + np.einsum("nra,nrb->ab", np.abs(J), np.abs(v_T))
    out[:, 3] = v_p.sum(0)
    mag[:, 3] = a_p.sum(0)
    if mutate == "v_t=W^T.sum":
        out[:, 3] = view_of(u)[0].T @ out[:, 3]
    return out, mag


# ---- rounding bounds of the rigid identities (tests/test_gpu_pose.py) -------------------------------------------------
# Moving the world by a twist equals moving the camera by its inverse:
#   rotation     <v_W, W [w]x> = sum_i v_means_i . (w x m_i) + sum_i v_quats_i . dq_i,   dq = 1/2 (0, w) (x) q
#   translation  v_t_view = W sum_i v_means_i                                            (W orthonormal)
# Both sides of a call come from the same compact sums through the same f32 program up to the intermediates
# (v_p parts, J, T, V, M, v_cov) of splat_projection_vjp, which the pose kernel and the parameter kernel evaluate with
# the same IEEE operations (no contraction, no reassociation): only the operations behind those separate them.
# Counted on the expression trees, in units of 2^-24 times the sums of absolute terms (`identity_mags`):
#   position terms   pose kernel: v_p = vpj + v_t (+ v_z) 2, the product with mean 1, the sum with J^T v_T 1  -> 4
#                    parameter kernel: W^T vpj 3, W^T v_t 3, their sum 1 (+ v_z W row 2: 2)                     -> 7 (9)
#   covariance terms pose kernel: v_T = (v_cov T) V^T + (v_cov^T T) V  3 + 3 + 1, J^T v_T 3, the sum 1         -> 11
#                    parameter kernel: v_V = (T^T v_cov) T 6, the c sums 1, v_M = 2 sym(v_V) M 3, v_R = v_M S 1,
#                    the quaternion VJP 6, and R(q) of a quaternion normalised in f32 is orthonormal to 4 u    -> 21,
#                    doubled: the VJP spreads v_R over four components (|q_i| <= 1) that dq gathers again      -> 42
#   the f32 store of the twelve words                                                                          -> 1
# K_ROT bounds every term by the larger class: 11 + 42 + 4 + 7 = 64.  Translation: 2 + 9 + 1, and W W^T = I to 2 u
# for a camera matrix rounded to f32 -> K_TR = 14.
K_ROT = 64.0
K_TR = 14.0


def identity_mags(u, means, log_scales, quats, v_xy, v_conic, omegas, v_z=None, v_comp=None, gids=None):
    """(mag_rot [len(omegas)], mag_tr [3]): the float64 sums of absolute terms the two identities are made of, every
    product chain taken over absolute values (|T| = |J| |W|, |V| = |M| |M|^T, |v_cov| = |conic| |G| |conic| ...)."""
    if gids is not None:
        gids = np.asarray(gids).astype(np.int64)
        means, log_scales, quats = (np.asarray(a)[gids] for a in (means, log_scales, quats))
    omegas = np.asarray(omegas, np.float64)
    if np.asarray(means).shape[0] == 0:
        return np.zeros(len(omegas)), np.zeros(3)
    W, f, pc, img, p, scale, R, M, V = A._parts(u, means, log_scales, quats)
    n = p.shape[0]
    v_xy = np.abs(np.asarray(v_xy, np.float64).reshape(n, 2))
    v_conic = np.abs(np.asarray(v_conic, np.float64).reshape(n, 3))
    cov, blurred = A.cov2d64(u, means, log_scales, quats)
    det = blurred[:, 0, 0] * blurred[:, 1, 1] - blurred[:, 0, 1] ** 2
    conic = np.abs(np.stack([np.stack([blurred[:, 1, 1], -blurred[:, 0, 1]], -1),
                             np.stack([-blurred[:, 1, 0], blurred[:, 0, 0]], -1)], 1) / det[:, None, None])
    G = np.stack([np.stack([v_conic[:, 0], 0.5 * v_conic[:, 1]], -1),
                  np.stack([0.5 * v_conic[:, 1], v_conic[:, 2]], -1)], 1)
    v_cov = conic @ G @ conic
    if v_comp is not None:
        comp = A.comp_from(cov, blurred)
        inv_det = np.abs(conic[:, 0, 0] * conic[:, 1, 1]) + conic[:, 0, 1] ** 2
        v_sqr = np.where(comp > 0, np.abs(np.asarray(v_comp, np.float64)) * 0.5 / (comp + 1e-6), 0.0)
        v_cov = v_cov + v_sqr[:, None, None] * (np.abs(1 - comp * comp)[:, None, None] * conic
                                                + A.COV_BLUR * inv_det[:, None, None] * np.eye(2))
    z = np.abs(p[:, 2])
    pa = np.abs(p)
    rw = 1.0 / z
    a0, a1 = f[0] * v_xy[:, 0], f[1] * v_xy[:, 1]
    vpj = np.stack([a0 * rw, a1 * rw, (a0 * pa[:, 0] + a1 * pa[:, 1]) * rw * rw], -1)
    Ja = np.abs(A._jac(f, p, p[:, 0], p[:, 1]))
    Wa = np.abs(W)
    Ta = Ja @ Wa
    Va = np.abs(M) @ np.transpose(np.abs(M), (0, 2, 1))
    vT = 2.0 * v_cov @ Ta @ Va
    vJ = vT @ Wa.T
    rz2, rz3 = 1 / z ** 2, 1 / z ** 3
    v_t = np.stack([f[0] * rz2 * vJ[:, 0, 2], f[1] * rz2 * vJ[:, 1, 2],
                    f[0] * rz2 * vJ[:, 0, 0] + 2 * f[0] * pa[:, 0] * rz3 * vJ[:, 0, 2]
                    + f[1] * rz2 * vJ[:, 1, 1] + 2 * f[1] * pa[:, 1] * rz3 * vJ[:, 1, 2]], -1)
    a_p = vpj + v_t
    if v_z is not None:
        a_p[:, 2] += np.abs(np.asarray(v_z, np.float64).reshape(n))
    ma = np.abs(np.asarray(means, np.float64))
    mag_rot = []
    for w in omegas:
        X = Wa @ np.abs(hat(w))                                   # |W| |[w]x|
        mag_rot.append(float(np.einsum("na,ab,nb->", a_p, X, ma) + np.einsum("nra,nrb,ab->", Ja, vT, X)))
    mag_tr = (Wa @ Wa.T) @ a_p.sum(0)
    return np.array(mag_rot), mag_tr


def identity_sides(u, means, quats, v_viewmat, v_means, v_quats, omegas):
    """float64: (lhs_rot, rhs_rot [len(omegas)], lhs_tr, rhs_tr [3]) of the two identities from a call's outputs."""
    W, t = view_of(u)
    m = np.asarray(means, np.float64)
    q = np.asarray(quats, np.float64)
    vm = np.asarray(v_means, np.float64)
    vq = np.asarray(v_quats, np.float64)
    vv = np.asarray(v_viewmat, np.float64).reshape(3, 4)
    lhs, rhs = [], []
    for w in np.asarray(omegas, np.float64):
        lhs.append(float((vv[:, :3] * (W @ hat(w))).sum()))
        dq = 0.5 * np.concatenate([-(q[:, 1:] @ w)[:, None], q[:, :1] * w[None, :] + np.cross(w[None, :], q[:, 1:])], 1)
        rhs.append(float((vm * np.cross(w[None, :], m)).sum() + (vq * dq).sum()))
    return np.array(lhs), np.array(rhs), vv[:, 3].copy(), W @ vm.sum(0)


# ---- se3 helpers in numpy (float64), independent of brush_amd.pose
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def expm_series(A4, terms=40):
    """Matrix exponential by scaling and squaring of the Taylor series (float64)."""
    A4 = np.asarray(A4, np.float64)
    s = max(0, int(np.ceil(np.log2(max(np.abs(A4).sum(1).max(), 1e-300)))) + 4)
    B = A4 / (2.0 ** s)
    E, term = np.eye(A4.shape[0]), np.eye(A4.shape[0])
    for k in range(1, terms):
        term = term @ B / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def twist_matrix(delta):
    d = np.asarray(delta, np.float64)
    X = np.zeros((4, 4))
    X[:3, :3] = hat(d[:3])
    X[:3, 3] = d[3:]
    return X


# ---- the pose-fit problem shared by the CPU rehearsal (oracle + pose_grad64) and the GPU test (render_splats_pose)
FIT_W, FIT_H = 64, 48
FIT_STEPS = 200
FIT_LR = (3e-3, 1.5e-2)                      # rotation [rad], translation [world units] per Adam step
FIT_DELTA = (0.03, -0.04, 0.05, 0.15, -0.1, 0.2)  # the perturbation: 4 degrees, 0.27 units at 8 units from the scene


def fit_problem():
    """A fixed SH-degree-0 cloud of 64 splats, 4 units wide and 7 deep, 8 units in front of the reference test camera.
    The depth spread is what makes the fit well conditioned: a shallow cloud (tried first: 3 units deep) leaves a
    valley between panning and translating that Adam crawls along, and its rehearsal stopped at a third of the
    initial rotation error."""
    rng = np.random.default_rng(1234)
    n = 64
    means = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-3.5, 3.5, n)], 1)
    means = means.astype(np.float32)
    log_scales = np.log(rng.uniform(0.15, 0.4, (n, 3))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    quats = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sh = rng.uniform(-1.5, 1.5, (n, 1, 3)).astype(np.float32)
    raw_opac = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return dict(means=means, log_scales=log_scales, quats=quats, sh=sh, raw_opac=raw_opac)


def pose_errors(M, M_true):
    """(rotation angle [rad], translation distance) between two rigid 4x4 matrices."""
    M, M_true = np.asarray(M, np.float64), np.asarray(M_true, np.float64)
    Rd = M[:3, :3] @ M_true[:3, :3].T
    ang = float(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)))
    return ang, float(np.linalg.norm(M[:3, 3] - M_true[:3, 3]))


def fit_pose(loss_fn, M_true, steps=FIT_STEPS, lr=FIT_LR, delta0=FIT_DELTA):
    """torch Adam (betas 0.9 / 0.999, eps 1e-15) on a twist, viewmat = apply_delta(M_true, delta) cast to float32,
    from delta0; loss_fn(viewmat) -> a scalar tensor differentiable with respect to viewmat (a [4,4] float32 CPU
    tensor).  Returns (first (angle, distance) error, last, losses)."""
    import torch

    from brush_amd.pose import apply_delta

    omega = torch.tensor(delta0[:3], dtype=torch.float64, requires_grad=True)
    tau = torch.tensor(delta0[3:], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([{"params": [omega], "lr": lr[0]}, {"params": [tau], "lr": lr[1]}], eps=1e-15)
    base = torch.as_tensor(np.asarray(M_true, np.float64))
    losses, first = [], None
    for _ in range(steps):
        M = apply_delta(base, torch.cat([omega, tau]))
        if first is None:
            first = pose_errors(M.detach().numpy(), M_true)
        opt.zero_grad()
        loss = loss_fn(M.to(torch.float32))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        last = pose_errors(apply_delta(base, torch.cat([omega, tau])).numpy(), M_true)
    return first, last, losses
