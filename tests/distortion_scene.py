"""The end-to-end scenes of the depth-distortion tests and what both the CPU and the GPU test need of them: a seeded
cloud in front of an off-centre, rotated camera of tests/camera_cases.py, the kernel-input `case` (tests/contrib_cases.py's
format) of a finished forward's aux, the float64 autograd projection that carries compact-row sums to the parameters,
and the exclusion rule.

EXCLUSION: a splat with a record within RISK allowances of one of the walk's thresholds (distortion_ref64.walk: risk) may
be decided differently in float32 than in the float64 reference; it is left out of the comparison of the gradients.  At
most MAX_EXCLUDED of the visible splats may be left out; both tests assert that cap (the CPU test through the oracle's
projection, the GPU test on the aux it reads back).
"""
import numpy as np

from tests import aa_ref64 as A
from tests import camera_cases as CamC
from tests import distortion_ref64 as R

W, H = 48, 40            # 3 x 3 tiles, the last row half outside the frame (48 is a whole number of tiles)
N = 200
CAMERA = "general"       # rotated about a skew axis, off-centre principal point, fov_y scaled
SEED = 3                 # picked in tests/test_distortion_cpu.py: the exclusion cap holds under the oracle's projection
RISK = 8.0
MAX_EXCLUDED = 0.05
K_PROJ = 128.0           # roundings of the parameter backward's chain: twice aa_ref64.K_COV (the projection recomputed,
                         # then its VJP), at the magnitude of the terms it sums


def _camera_space_cloud(rng, n, w, h, f, pc, z_lo, z_hi, s_lo, s_hi, o_hi):
    z = rng.uniform(z_lo, z_hi, n)
    px, py = rng.uniform(-4.0, w + 4.0, n), rng.uniform(-4.0, h + 4.0, n)
    p = np.stack([(px - pc[0]) / f[0] * z, (py - pc[1]) / f[1] * z, z], 1)
    s = rng.uniform(s_lo, s_hi, n) * z / f[0]  # s_lo .. s_hi pixels on the screen
    scales = np.stack([s, s * rng.uniform(0.5, 1.0, n), s * rng.uniform(0.1, 0.5, n)], 1)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    o = rng.uniform(0.05, o_hi, n)
    return p, scales, q, np.log(o / (1.0 - o))


def _to_world(p_cam, q_cam, m):
    """Camera-space points and (w, x, y, z) rotations to the world of the float64 world-to-camera matrix m."""
    inv = np.linalg.inv(m)
    means = p_cam @ inv[:3, :3].T + inv[:3, 3]
    quats = CamC.quat_mul_wxyz(CamC.quat_wxyz_of(inv[:3, :3]), q_cam)
    return means, quats


def lens(w=W, h=H, camera=CAMERA):
    """(focal [2], pixel centre [2]) of the camera on a w x h frame, float64."""
    u = CamC.oracle_uniforms(camera, w, h, 0)
    return np.asarray(u["focal"], np.float64), np.asarray(u["pixel_center"], np.float64)


def scene(seed=SEED, n=N, w=W, h=H, camera=CAMERA):
    """The cloud (float32 arrays: means, log_scales, quats (unit), sh [n,1,3], raw_opac) of about n splats, opacities
    at most 0.9, in front of `camera`, between 3 and 9 units deep, 1.5 to 6 pixels wide."""
    rng = np.random.default_rng(9000 + seed)
    f, pc = lens(w, h, camera)
    p, scales, q, raw = _camera_space_cloud(rng, n, w, h, f, pc, 3.0, 9.0, 1.5, 6.0, 0.9)
    means, quats = _to_world(p, q, CamC.matrix64(camera, w, h))
    quats = quats.astype(np.float32)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True).astype(np.float32)
    return dict(means=means.astype(np.float32), log_scales=np.log(scales).astype(np.float32), quats=quats,
                sh=rng.uniform(-1.0, 1.0, (n, 1, 3)).astype(np.float32), raw_opac=raw.astype(np.float32))


def smooth_scene(w=32, h=32, camera=CAMERA):
    """Five large faint splats that cover the whole frame with alpha well above 1/255 and leave T far above the stop:
    L is smooth in the means (no threshold crossing inside a finite difference)."""
    rng = np.random.default_rng(77)
    f, pc = lens(w, h, camera)
    n = 5
    z = np.array([4.0, 5.0, 6.5, 8.0, 9.5])
    px, py = rng.uniform(8.0, w - 8.0, n), rng.uniform(8.0, h - 8.0, n)
    p = np.stack([(px - pc[0]) / f[0] * z, (py - pc[1]) / f[1] * z, z], 1)
    s = rng.uniform(30.0, 45.0, n) * z / f[0]
    scales = np.stack([s, s * 0.9, s * 0.6], 1)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    means, quats = _to_world(p, q, CamC.matrix64(camera, w, h))
    quats = quats.astype(np.float32)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True).astype(np.float32)
    o = np.array([0.25, 0.3, 0.2, 0.35, 0.3])
    return dict(means=means.astype(np.float32), log_scales=np.log(scales).astype(np.float32), quats=quats,
                sh=np.full((n, 1, 3), 0.3, np.float32), raw_opac=np.log(o / (1 - o)).astype(np.float32))


def case_from_aux(aux, w, h, n):
    """The kernel inputs of a finished forward (a dict of numpy arrays named as RenderAux's fields) in
    tests/contrib_cases.py's format."""
    v = int(np.asarray(aux["num_visible"]).reshape(-1)[0])
    isect = np.asarray(aux["compact_gid_from_isect"]).astype(np.int32)
    bins = np.asarray(aux["tile_bins"]).astype(np.int32)
    return dict(name="scene", w=w, h=h, n=n, projected=np.asarray(aux["projected_splats"], np.float32),
                tile_bins=bins, isect=isect, num_isect=int(bins[..., 1].max()) if bins.size else 0,
                g_from_c=np.asarray(aux["global_from_compact_gid"]).astype(np.int32), num_visible=v)


def view_z(viewmat, means):
    """Camera-space z of every mean in float32 with the projection's own association (splat_math.hpp: to_view);
    viewmat: the 16 column-major words."""
    vm = np.asarray(list(viewmat), np.float32)
    m = np.asarray(means, np.float32)
    return ((vm[2] * m[:, 0] + vm[6] * m[:, 1]) + vm[10] * m[:, 2]) + vm[14]


def oracle_case(cloud, w=W, h=H, camera=CAMERA):
    """(case, compact_depth [n] f32) of the cloud projected, binned and sorted by the CPU oracle (plain mode)."""
    from oracle import oracle as O

    u = CamC.oracle_uniforms(camera, w, h, 0)
    _, aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"])
    n = cloud["means"].shape[0]
    case = case_from_aux(aux, w, h, n)
    z = np.zeros(n, np.float32)
    v = case["num_visible"]
    z[:v] = view_z(u["viewmat"], cloud["means"])[case["g_from_c"][:v]]
    return case, z


def excluded(ref, num_visible):
    """(mask [n] by compact id of the splats left out, their share of the visible ones)."""
    bad = ref["risk"] < RISK
    bad[num_visible:] = False
    return bad, float(bad[:num_visible].mean()) if num_visible else 0.0


def project64(u, cloud, antialiased):
    """float64 autograd projection of the whole cloud: returns (q, params), q [N,7] the quantities the compact-row
    words are gradients at (mean2d x, y, conic a, b, c, the drawn opacity, view z) as torch tensors of the leaf
    tensors params = (means, log_scales, quats, raw_opac).  calc_cov2d with the Jacobian at the unclamped p_view (the
    scenes keep every splat inside the clamp, asserted) and the 0.3 px^2 blur; checked against aa_ref64.cov2d64."""
    import torch

    Wm, tv, f, pc, img = A._view(u)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    means, ls, quats, raw = (t(cloud[k]).requires_grad_(True) for k in ("means", "log_scales", "quats", "raw_opac"))
    Wt, f_t = t(Wm), t(f)
    p = means @ Wt.T + t(tv)
    z = p[:, 2]
    w_, x, y, zq = (quats[:, i] for i in range(4))
    Rm = torch.stack([torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w_ * zq), 2 * (x * zq + w_ * y)], -1),
                      torch.stack([2 * (x * y + w_ * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w_ * x)], -1),
                      torch.stack([2 * (x * zq - w_ * y), 2 * (y * zq + w_ * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    M = Rm * torch.exp(ls)[:, None, :]
    V = M @ M.transpose(1, 2)
    zero = torch.zeros_like(z)
    J = torch.stack([torch.stack([f_t[0] / z, zero, -f_t[0] * p[:, 0] / (z * z)], -1),
                     torch.stack([zero, f_t[1] / z, -f_t[1] * p[:, 1] / (z * z)], -1)], 1)
    T = J @ Wt
    cov = T @ V @ T.transpose(1, 2)
    blurred = cov + A.COV_BLUR * torch.eye(2, dtype=torch.float64)
    assert not A.clamp_active(u, cloud["means"]).any()
    ref_cov, ref_blur = A.cov2d64(u, cloud["means"], cloud["log_scales"], cloud["quats"])
    assert np.allclose(cov.detach().numpy(), ref_cov, rtol=1e-11, atol=1e-13)
    det = blurred[:, 0, 0] * blurred[:, 1, 1] - blurred[:, 0, 1] * blurred[:, 1, 0]
    conic = torch.stack([blurred[:, 1, 1] / det, -blurred[:, 0, 1] / det, blurred[:, 0, 0] / det], -1)
    opac = torch.sigmoid(raw)
    if antialiased:
        det_o = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
        opac = opac * torch.sqrt(torch.clamp(det_o / det, min=0.0))
    mean2d = torch.stack([f_t[0] * p[:, 0] / z + pc[0], f_t[1] * p[:, 1] / z + pc[1]], -1)
    q = torch.cat([mean2d, conic, opac[:, None], z[:, None]], 1)
    return q, (means, ls, quats, raw)


def push_rows(u, cloud, antialiased, rows, tol_rows, g_from_c, num_visible):
    """The compact-row sums `rows` [n,7] (and their allowances) carried to the parameters: dict name -> (gradient,
    allowance), float64, for v_means, v_scales, v_quats, v_opac by GLOBAL id.  Every splat's seven quantities depend on
    its own parameters only, so the gradient of the sum over splats of quantity j is its per-splat Jacobian D_j:
    gradient = sum_j rows_j D_j, allowance = sum_j tol_rows_j |D_j| + K_PROJ U sum_j |rows_j D_j|."""
    import torch

    n = cloud["means"].shape[0]
    q, params = project64(u, cloud, antialiased)
    r_g, t_g = np.zeros((n, 7)), np.zeros((n, 7))
    gids = np.asarray(g_from_c[:num_visible]).astype(np.int64)
    r_g[gids], t_g[gids] = rows[:num_visible], tol_rows[:num_visible]
    names = ("v_means", "v_scales", "v_quats", "v_opac")
    out = {k: [np.zeros(tuple(p.shape)), np.zeros(tuple(p.shape))] for k, p in zip(names, params)}
    for j in range(7):
        D = torch.autograd.grad(q[:, j].sum(), params, retain_graph=True, allow_unused=True)
        for k, p, d in zip(names, params, D):
            if d is None:
                continue
            d = d.numpy()
            rj = r_g[:, j].reshape((n,) + (1,) * (d.ndim - 1))
            tj = t_g[:, j].reshape((n,) + (1,) * (d.ndim - 1))
            out[k][0] += rj * d
            out[k][1] += tj * np.abs(d) + K_PROJ * A.U * np.abs(rj * d)
    return {k: (v[0], v[1]) for k, v in out.items()}
