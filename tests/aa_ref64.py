"""float64 restatement of the antialiased mode's per-splat math (include/brush_hip.h: BRUSH_AUX_ANTIALIASED).

* cov2d64: calc_cov2d (splat_math.hpp, helpers.wgsl:124-158) with its frustum clamp, before and after the 0.3 px^2 blur;
* comp64: sqrt(max(0, det(S) / det(S + 0.3 I))), 0 where det(S) <= 0;
* comp_vjp64: the VJP from v_comp to (means, log_scales, normalised quats) exactly as splat_vjp.hpp computes it:
  v_sqr = v_comp 0.5 / (comp + 1e-6), d comp^2 / d(S + 0.3 I) = (1 - comp^2) conic - 0.3 det(conic) I, then the
  projection chain of splat_projection_vjp with the Jacobian at the UNCLAMPED p_view;
* word8_bound: a forward-error bound of the kernel's f32 opacity word sigmoid(raw) * comp, derived from the
  expression (operation counts x 2^-24 x the float64 magnitudes of the terms), not from any GPU output.

Everything is vectorised over splats; `u` is a BrushUniforms (or anything with viewmat / focal / pixel_center /
img_size)."""
import numpy as np

U = 2.0 ** -24
COV_BLUR = 0.3


def _view(u):
    vm = np.array(list(u.viewmat), np.float64)
    W = np.array([[vm[c * 4 + r] for c in range(3)] for r in range(3)])
    t = vm[12:15]
    f = np.array(list(u.focal), np.float64)
    pc = np.array(list(u.pixel_center), np.float64)
    img = np.array(list(u.img_size), np.float64)
    return W, t, f, pc, img


def rotmat(q):
    """helpers.wgsl:74-109, q = (w, x, y, z) [N,4] -> [N,3,3] (row-major)."""
    w, x, y, z = (q[:, i] for i in range(4))
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _lims(f, pc, img):
    tan_fov = 0.5 * img / f
    return (img - pc) / f + 0.3 * tan_fov, pc / f + 0.3 * tan_fov


def _parts(u, means, log_scales, quats):
    W, tv, f, pc, img = _view(u)
    m = np.asarray(means, np.float64)
    p = m @ W.T + tv
    scale = np.exp(np.asarray(log_scales, np.float64))
    R = rotmat(np.asarray(quats, np.float64))
    M = R * scale[:, None, :]
    V = M @ np.transpose(M, (0, 2, 1))
    return W, f, pc, img, p, scale, R, M, V


def _jac(f, p, tx, ty):
    """[N,2,3] Jacobian of the projection with the (clamped or not) tangent-plane position (tx, ty)."""
    z = p[:, 2]
    J = np.zeros((p.shape[0], 2, 3))
    J[:, 0, 0] = f[0] / z
    J[:, 1, 1] = f[1] / z
    J[:, 0, 2] = -f[0] * tx / (z * z)
    J[:, 1, 2] = -f[1] * ty / (z * z)
    return J


def clamp_active(u, means):
    W, tv, f, pc, img = _view(u)
    p = np.asarray(means, np.float64) @ W.T + tv
    lp, ln = _lims(f, pc, img)
    r = p[:, :2] / p[:, 2:3]
    return ((r < -ln) | (r > lp)).any(axis=1)


def cov2d64(u, means, log_scales, quats):
    """(unblurred [N,2,2], blurred [N,2,2]) of calc_cov2d."""
    W, f, pc, img, p, scale, R, M, V = _parts(u, means, log_scales, quats)
    lp, ln = _lims(f, pc, img)
    z = p[:, 2]
    tx = z * np.clip(p[:, 0] / z, -ln[0], lp[0])
    ty = z * np.clip(p[:, 1] / z, -ln[1], lp[1])
    T = _jac(f, p, tx, ty) @ W
    cov = T @ V @ np.transpose(T, (0, 2, 1))
    return cov, cov + COV_BLUR * np.eye(2)


def comp_from(cov, blurred):
    det_o = cov[:, 0, 0] * cov[:, 1, 1] - cov[:, 0, 1] * cov[:, 1, 0]
    det = blurred[:, 0, 0] * blurred[:, 1, 1] - blurred[:, 0, 1] * blurred[:, 1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(det_o > 0, det_o / det, 0.0)
    return np.sqrt(np.maximum(r, 0.0))


def comp64(u, means, log_scales, quats):
    return comp_from(*cov2d64(u, means, log_scales, quats))


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-np.asarray(raw, np.float64)))


def comp_vjp64(u, means, log_scales, quats, v_comp):
    """(v_means [N,3], v_log_scales [N,3], v_quats [N,4]) of sum(v_comp * comp) as the backward computes them."""
    W, f, pc, img, p, scale, R, M, V = _parts(u, means, log_scales, quats)
    cov, blurred = cov2d64(u, means, log_scales, quats)
    comp = comp_from(cov, blurred)
    det = blurred[:, 0, 0] * blurred[:, 1, 1] - blurred[:, 0, 1] ** 2
    conic = np.stack([np.stack([blurred[:, 1, 1], -blurred[:, 0, 1]], -1),
                      np.stack([-blurred[:, 1, 0], blurred[:, 0, 0]], -1)], 1) / det[:, None, None]
    inv_det = conic[:, 0, 0] * conic[:, 1, 1] - conic[:, 0, 1] ** 2
    v_sqr = np.where(comp > 0, np.asarray(v_comp, np.float64) * 0.5 / (comp + 1e-6), 0.0)
    v_cov = v_sqr[:, None, None] * ((1 - comp * comp)[:, None, None] * conic
                                    - COV_BLUR * inv_det[:, None, None] * np.eye(2))
    # projection chain (splat_projection_vjp) with J at the unclamped p_view
    J = _jac(f, p, p[:, 0], p[:, 1])
    T = J @ W
    Tt = np.transpose(T, (0, 2, 1))
    v_V = Tt @ v_cov @ T
    v_T = 2.0 * v_cov @ T @ V
    v_J = v_T @ W.T
    z = p[:, 2]
    rz, rz2, rz3 = 1 / z, 1 / z ** 2, 1 / z ** 3
    v_t = np.stack([-f[0] * rz2 * v_J[:, 0, 2], -f[1] * rz2 * v_J[:, 1, 2],
                    -f[0] * rz2 * v_J[:, 0, 0] + 2 * f[0] * p[:, 0] * rz3 * v_J[:, 0, 2]
                    - f[1] * rz2 * v_J[:, 1, 1] + 2 * f[1] * p[:, 1] * rz3 * v_J[:, 1, 2]], -1)
    v_means = v_t @ W
    v_M = (v_V + np.transpose(v_V, (0, 2, 1))) @ M
    v_scales = (R * v_M).sum(axis=1) * scale
    v_R = v_M * scale[:, None, :]
    q = np.asarray(quats, np.float64)
    w, x, y, zq = (q[:, i] for i in range(4))

    def G(a, b):  # WGSL v_R[a][b] = column a, row b
        return v_R[:, b, a]

    v_q = np.stack([
        2 * (x * (G(1, 2) - G(2, 1)) + y * (G(2, 0) - G(0, 2)) + zq * (G(0, 1) - G(1, 0))),
        2 * (-2 * x * (G(1, 1) + G(2, 2)) + y * (G(0, 1) + G(1, 0)) + zq * (G(0, 2) + G(2, 0)) + w * (G(1, 2) - G(2, 1))),
        2 * (x * (G(0, 1) + G(1, 0)) - 2 * y * (G(0, 0) + G(2, 2)) + zq * (G(1, 2) + G(2, 1)) + w * (G(2, 0) - G(0, 2))),
        2 * (x * (G(0, 2) + G(2, 0)) + y * (G(1, 2) + G(2, 1)) - 2 * zq * (G(0, 0) + G(1, 1)) + w * (G(0, 1) - G(1, 0))),
    ], -1)
    return v_means, v_scales, v_q


# ---- forward-error bound of word 8 ------------------------------------------------------------------------------
K_COV = 64.0   # calc_cov2d's chain, counted on the kernel's expression tree: p_view 6, rz / x rz / t 4, J entries 9,
#                T = J W 3 (12), R(q) 4, M = R s with det_expf 3 (7), V = M M^T 5 (19), T V 5 (36), (T V) T^T 5 (53)
K_SIG = 8.0    # det_sigmoid = 1 / (1 + det_expf(-x)): the exponential (<= 4 ulp relative), the sum and the division


def word8_bound(u, means, log_scales, quats, raw_opac):
    """(want [N] = sigmoid(raw) comp in float64, bound [N]) for the kernel's f32 word 8.

    Every cov2d term is a sum of products whose f32 evaluation errs by at most K_COV U times the same sum taken over
    absolute values (|T| |V| |T|^T, with |p_view| replaced by the magnitudes it is summed from); the two determinants
    add 3 U of their products, the ratio, the square root and the final product 1 U each.  Where the error of det(S)
    reaches det(S) itself the kernel's comp can be anything from 0 to the largest value the bounds allow."""
    W, f, pc, img, p, scale, R, M, V = _parts(u, means, log_scales, quats)
    cov, blurred = cov2d64(u, means, log_scales, quats)
    comp = comp_from(cov, blurred)
    sig = sigmoid64(raw_opac)
    want = sig * comp
    lp, ln = _lims(f, pc, img)
    m = np.asarray(means, np.float64)
    tv = np.array(list(u.viewmat), np.float64)[12:15]
    pabs = np.abs(m) @ np.abs(W).T + np.abs(tv)
    z = p[:, 2]
    txa = np.abs(z) * np.minimum(pabs[:, 0] / np.abs(z), max(lp[0], ln[0]))
    tya = np.abs(z) * np.minimum(pabs[:, 1] / np.abs(z), max(lp[1], ln[1]))
    Ta = np.abs(_jac(np.abs(f), np.abs(p), txa, tya)) @ np.abs(W)
    Va = np.abs(M) @ np.abs(np.transpose(M, (0, 2, 1)))
    cov_abs = Ta @ Va @ np.transpose(Ta, (0, 2, 1))
    e = K_COV * U * cov_abs
    eb = e + U * (np.abs(blurred))  # + the rounding of the blur's addition
    a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    ab, bb, cb = blurred[:, 0, 0], blurred[:, 0, 1], blurred[:, 1, 1]
    det_o, det = a * c - b * b, ab * cb - bb * bb
    e_do = np.abs(a) * e[:, 1, 1] + np.abs(c) * e[:, 0, 0] + 2 * np.abs(b) * e[:, 0, 1] + 3 * U * (np.abs(a * c) + b * b)
    e_d = np.abs(ab) * eb[:, 1, 1] + np.abs(cb) * eb[:, 0, 0] + 2 * np.abs(bb) * eb[:, 0, 1] + 3 * U * (np.abs(ab * cb) + bb * bb)
    e_d = e_d * 1.01  # second-order terms of the products of errors
    e_do = e_do * 1.01
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = 0.5 * (e_do / det_o + e_d / det + U) + 2 * U
        resolved = (det_o > e_do) & (det > e_d)
        comp_err = np.where(resolved, comp * rel * 1.01,
                            np.sqrt(np.maximum(det_o + e_do, 0.0) / np.maximum(det - e_d, 1e-300)))
    bound = sig * comp_err + want * (K_SIG + 1) * U + 1e-45
    return want, bound
