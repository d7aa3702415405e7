"""float64 restatement of the exposure kernels (include/brush_hip.h: brush_exposure_forward, brush_exposure_backward,
brush_exposure_backward_adam; brush_amd/csrc/exposure.hip), with the sum of the absolute values of the terms of every
output beside it: the scale the f32 kernels' rounding bounds are stated in.

E = [A | b], 12 words row-major; img [h,w,4] premultiplied (r, g, b, alpha):
    out_c = A[c,0] r + A[c,1] g + A[c,2] b + alpha b_c        out_alpha = alpha
"""
import numpy as np

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15


def _e34(E):
    return np.asarray(E, dtype=np.float64).reshape(3, 4)


def forward(img, E):
    """(out [h,w,4], sum |terms| [h,w,4]); the alpha channel is a copy (its |terms| is |alpha|)."""
    p, E = np.asarray(img, dtype=np.float64), _e34(E)
    out, mag = np.empty_like(p), np.empty_like(p)
    out[..., :3] = p @ E.T               # p_k E[c,k] over k = 0..3, p_3 = alpha
    mag[..., :3] = np.abs(p) @ np.abs(E).T
    out[..., 3], mag[..., 3] = p[..., 3], np.abs(p[..., 3])
    return out, mag


def backward_image(v_out, E):
    """(v_pred [h,w,4], sum |terms| [h,w,4]) from v' = d L / d out."""
    v, E = np.asarray(v_out, dtype=np.float64), _e34(E)
    vp, mag = np.empty_like(v), np.empty_like(v)
    vp[..., :3] = v[..., :3] @ E[:, :3]
    mag[..., :3] = np.abs(v[..., :3]) @ np.abs(E[:, :3])
    vp[..., 3] = v[..., 3] + v[..., :3] @ E[:, 3]
    mag[..., 3] = np.abs(v[..., 3]) + np.abs(v[..., :3]) @ np.abs(E[:, 3])
    return vp, mag


def backward_exposure(img, v_out):
    """(v_E [3,4], sum |terms| [3,4]): v_E[c,k] = sum_pixels v'_c p_k."""
    p = np.asarray(img, dtype=np.float64).reshape(-1, 4)
    v = np.asarray(v_out, dtype=np.float64).reshape(-1, 4)[:, :3]
    return v.T @ p, np.abs(v).T @ np.abs(p)


def adam_step(E, m1, m2, grad, lr, reg, time, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One Adam step of a view's E from the stored f32 state, in float64: the coupled penalty reg (E - [I|0]) is added
    to `grad`; bias corrections 1 - beta^time with a 1-based `time`.  The hyper-parameters are taken as the f32 values
    the ABI's struct carries.  Returns (E, m1, m2) as float64 [3,4]."""
    f = lambda x: float(np.float32(x))
    lr, reg, beta1, beta2, eps = f(lr), f(reg), f(beta1), f(beta2), f(eps)
    E, m1, m2 = _e34(E), _e34(m1), _e34(m2)
    g = _e34(grad) + reg * (E - IDENTITY)
    m1 = beta1 * m1 + (1.0 - beta1) * g
    m2 = beta2 * m2 + (1.0 - beta2) * g * g
    mhat = m1 / (1.0 - beta1 ** time)
    vhat = m2 / (1.0 - beta2 ** time)
    return E - lr * mhat / (np.sqrt(vhat) + eps), m1, m2
