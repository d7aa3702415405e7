"""float64 restatement of the bilateral-grid kernels (include/brush_hip.h: brush_bilagrid_forward, _backward,
_backward_adam; brush_amd/csrc/bilagrid.hip), with the sum of the absolute values of the terms of every output beside
it: the scale the kernels' rounding bounds are stated in.

Definitions (all f32, round to nearest, never contracted, in the order written).
Grid G[GL][GH][GW][12] float32, vertex-major; a vertex is the row-major 3x4 [A | b] of exposure_ref64; 2 <= GW, GH <= 64,
2 <= GL <= 8.  Pixel (x, y), exact in integers: w == 1: i0 = 0, fx = 0; otherwise n = x (GW-1), i0 = min(n div (w-1), GW-2),
fx = float(n - i0 (w-1)) / float(w-1); y, h, GH give j0, fy.  Guidance on p = (r, g, b, a):
lum = (0.299f r + 0.587f g) + 0.114f b; lc = lum > 0 ? min(lum, 1) : 0 (NaN gives 0); z = lc float(GL-1),
k0 = min((int) z, GL-2), fz = z - float(k0); inside = lum > 0 && lum < 1.  lerp(a, b, f) = a + f (b - a); per word,
L_k = lerp(lerp(G[k][j0][i0], G[k][j0][i0+1], fx), lerp(G[k][j0+1][i0], G[k][j0+1][i0+1], fx), fy) for k in {k0, k0+1},
M = lerp(L_k0, L_k0+1, fz), S = L_k0+1 - L_k0.  out_c = ((M[4c] r + M[4c+1] g) + M[4c+2] b) + a M[4c+3], out_a = a.
Backward: q = inside ? float(GL-1) sum_c v'_c (S[4c..4c+3] . p) : 0; v_r = sum_c M[4c] v'_c + 0.299f q (g, b alike);
v_a = v'_a + sum_c M[4c+3] v'_c; v_G[k][j][i][4c+m] = sum_pixels X Y Z v'_c p_m with the tent weights of fx, fy, fz.
TV(G) = sum over the axes of the mean over adjacent pairs and words of (G[v+e] - G[v])^2.

The coordinates i0, fx, j0, fy, k0, fz and `inside` are taken from the float32 definition with numpy float32 operations
in the same order, so a pixel near a cell boundary sits in the same cell here and in the kernel; everything after that
is float64.  `continuous=True` takes the luminance and fz in float64 instead: the differentiable functional the
gradient test differentiates.
"""
import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
LUMA = (0.299, 0.587, 0.114)
F = np.float32


def identity(shape):
    gw, gh, gl = shape
    return np.tile(IDENTITY, (gl, gh, gw, 1))


def axis_coords(w, g):
    """(i0 [w] int64, f [w] float32) of the pixels 0..w-1 along an axis of g vertices."""
    x = np.arange(w, dtype=np.int64)
    if w == 1:
        return np.zeros(1, np.int64), np.zeros(1, F)
    n = x * (g - 1)
    i0 = np.minimum(n // (w - 1), g - 2)
    return i0, (n - i0 * (w - 1)).astype(F) / F(w - 1)


def guidance(pred, gl, continuous=False):
    """(k0 [h,w] int64, fz [h,w], inside [h,w] bool)."""
    if continuous:
        p = np.asarray(pred, dtype=np.float64)
        lum = (LUMA[0] * p[..., 0] + LUMA[1] * p[..., 1]) + LUMA[2] * p[..., 2]
        z = np.clip(lum, 0.0, 1.0) * (gl - 1)
        k0 = np.minimum(np.floor(z).astype(np.int64), gl - 2)
        return k0, z - k0, (lum > 0) & (lum < 1)
    p = np.asarray(pred, dtype=F)
    with np.errstate(invalid="ignore"):
        lum = (F(0.299) * p[..., 0] + F(0.587) * p[..., 1]) + F(0.114) * p[..., 2]
        pos = lum > 0
        lc = np.where(pos, np.minimum(np.where(pos, lum, F(0)), F(1)), F(0)).astype(F)
        z = lc * F(gl - 1)
        k0 = np.minimum(z.astype(np.int64), gl - 2)
        fz = z - k0.astype(F)
        inside = pos & (lum < 1)
    assert z.dtype == F and fz.dtype == F
    return k0, fz, inside


def coords(pred, shape, continuous=False):
    """i0 [1,w], fx [1,w], j0 [h,1], fy [h,1], k0, fz, inside [h,w]; the fractions as float64 values."""
    gw, gh, gl = shape
    h, w = pred.shape[:2]
    i0, fx = axis_coords(w, gw)
    j0, fy = axis_coords(h, gh)
    k0, fz, inside = guidance(pred, gl, continuous)
    if continuous:  # the fractions of the continuous functional: the same integers, divided in float64
        fx = np.zeros(1) if w == 1 else (np.arange(w) * (gw - 1) - i0 * (w - 1)) / (w - 1)
        fy = np.zeros(1) if h == 1 else (np.arange(h) * (gh - 1) - j0 * (h - 1)) / (h - 1)
    return (i0[None, :], fx.astype(np.float64)[None, :], j0[:, None], fy.astype(np.float64)[:, None], k0,
            np.asarray(fz, dtype=np.float64), inside)


def _lerp(a, ma, b, mb, f):
    """lerp and the sum of |terms| (a, f b, -f a) of it."""
    return a + f * (b - a), ma + f * (ma + mb)


def slice_grid(pred, G, continuous=False):
    """(M, S, mag M, mag S), each [h,w,12]."""
    G = np.asarray(G, dtype=np.float64)
    shape = (G.shape[2], G.shape[1], G.shape[0])
    i0, fx, j0, fy, k0, fz, _ = coords(pred, shape, continuous)
    A = np.abs(G)
    L, mL = [], []
    for k in (k0, k0 + 1):
        a, ma = _lerp(G[k, j0, i0], A[k, j0, i0], G[k, j0, i0 + 1], A[k, j0, i0 + 1], fx[..., None])
        b, mb = _lerp(G[k, j0 + 1, i0], A[k, j0 + 1, i0], G[k, j0 + 1, i0 + 1], A[k, j0 + 1, i0 + 1], fx[..., None])
        c, mc = _lerp(a, ma, b, mb, fy[..., None])
        L.append(c), mL.append(mc)
    M, mM = _lerp(L[0], mL[0], L[1], mL[1], fz[..., None])
    return M, L[1] - L[0], mM, mL[0] + mL[1]


def forward(pred, G, continuous=False):
    """(out [h,w,4], sum |terms| [h,w,4]); the alpha channel is a copy."""
    p = np.asarray(pred, dtype=np.float64)
    M, _, mM, _ = slice_grid(pred, G, continuous)
    out, mag = np.empty_like(p), np.empty_like(p)
    out[..., :3] = np.einsum("hwcm,hwm->hwc", M.reshape(p.shape[:2] + (3, 4)), p)
    mag[..., :3] = np.einsum("hwcm,hwm->hwc", mM.reshape(p.shape[:2] + (3, 4)), np.abs(p))
    out[..., 3], mag[..., 3] = p[..., 3], np.abs(p[..., 3])
    return out, mag


def backward_image(pred, v_out, G, continuous=False):
    """(v_pred [h,w,4], sum |terms| [h,w,4]) from v' = d L / d out."""
    p, v = np.asarray(pred, dtype=np.float64), np.asarray(v_out, dtype=np.float64)
    gl = np.asarray(G).shape[0]
    _, _, _, _, _, _, inside = coords(pred, (np.asarray(G).shape[2], np.asarray(G).shape[1], gl), continuous)
    M, S, mM, mS = slice_grid(pred, G, continuous)
    hw = p.shape[:2]
    M, S, mM, mS = (t.reshape(hw + (3, 4)) for t in (M, S, mM, mS))
    vc, ac = v[..., :3], np.abs(v[..., :3])
    q = np.where(inside, (gl - 1) * np.einsum("hwc,hwcm,hwm->hw", vc, S, p), 0.0)
    mq = np.where(inside, (gl - 1) * np.einsum("hwc,hwcm,hwm->hw", ac, mS, np.abs(p)), 0.0)
    vp, mag = np.empty_like(p), np.empty_like(p)
    luma = np.asarray(LUMA if continuous else [float(F(c)) for c in LUMA])
    vp[..., :3] = np.einsum("hwc,hwcm->hwm", vc, M[..., :3]) + luma * q[..., None]
    mag[..., :3] = np.einsum("hwc,hwcm->hwm", ac, mM[..., :3]) + luma * mq[..., None]
    vp[..., 3] = v[..., 3] + np.einsum("hwc,hwc->hw", vc, M[..., 3])
    mag[..., 3] = np.abs(v[..., 3]) + np.einsum("hwc,hwc->hw", ac, mM[..., 3])
    return vp, mag


def backward_grid(pred, v_out, shape, continuous=False):
    """(v_G [GL,GH,GW,12], sum |terms|, reached [GL,GH,GW] bool: a pixel has a nonzero weight at the vertex)."""
    gw, gh, gl = shape
    p, v = np.asarray(pred, dtype=np.float64), np.asarray(v_out, dtype=np.float64)
    i0, fx, j0, fy, k0, fz, _ = coords(pred, shape, continuous)
    n = gl * gh * gw
    t = (v[..., :3, None] * p[..., None, :]).reshape(-1, 12)
    at = np.abs(t)
    out, mag, reached = np.zeros((n, 12)), np.zeros((n, 12)), np.zeros(n)
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                W = ((fx if di else 1.0 - fx) * (fy if dj else 1.0 - fy)) * (fz if dk else 1.0 - fz)
                idx = (((k0 + dk) * gh + (j0 + dj)) * gw + (i0 + di)).ravel()
                Wr = W.ravel()
                reached += np.bincount(idx, weights=(Wr > 0).astype(np.float64), minlength=n)
                for m in range(12):
                    out[:, m] += np.bincount(idx, weights=Wr * t[:, m], minlength=n)
                    mag[:, m] += np.bincount(idx, weights=Wr * at[:, m], minlength=n)
    return out.reshape(gl, gh, gw, 12), mag.reshape(gl, gh, gw, 12), reached.reshape(gl, gh, gw) > 0


def tv_terms(G):
    """The terms of TV(G), one per adjacent pair and word: (G[v+e] - G[v])^2 / the axis' pair count."""
    G = np.asarray(G, dtype=np.float64)
    return np.concatenate([(d * d).ravel() / d.size for d in (np.diff(G, axis=axis) for axis in (0, 1, 2))])


def tv(G):
    """(TV(G), sum |terms|): the squares are the terms."""
    total = float(tv_terms(G).sum())
    return total, total


def tv_grad(G):
    """(dTV/dG, sum |terms|), the shape of G."""
    G = np.asarray(G, dtype=np.float64)
    g, mag = np.zeros_like(G), np.zeros_like(G)
    for axis in (0, 1, 2):
        d = np.diff(G, axis=axis)
        c = 2.0 / d.size
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        g[tuple(hi)] += c * d
        g[tuple(lo)] -= c * d
        a = c * (np.abs(G[tuple(hi)]) + np.abs(G[tuple(lo)]))
        mag[tuple(hi)] += a
        mag[tuple(lo)] += a
    return g, mag


def adam_step(G, m1, m2, grad, lr, tv_weight, time, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One Adam step of a view's grid from the stored f32 state, in float64: tv_weight dTV/dG of the grid as given is
    added to `grad`; bias corrections 1 - beta^time with a 1-based `time`.  The hyper-parameters are taken as the f32
    values the ABI's struct carries.  Returns (G, m1, m2) as float64."""
    f = lambda x: float(F(x))
    lr, tv_weight, beta1, beta2, eps = f(lr), f(tv_weight), f(beta1), f(beta2), f(eps)
    G, m1, m2 = (np.asarray(t, dtype=np.float64) for t in (G, m1, m2))
    g = np.asarray(grad, dtype=np.float64) + tv_weight * tv_grad(G)[0]
    m1 = beta1 * m1 + (1.0 - beta1) * g
    m2 = beta2 * m2 + (1.0 - beta2) * g * g
    mhat = m1 / (1.0 - beta1 ** time)
    vhat = m2 / (1.0 - beta2 ** time)
    return G - lr * mhat / (np.sqrt(vhat) + eps), m1, m2


# ---- the backward kernel's partition of the image (bilagrid.hip: cell_first, slice_count) -----------------------------
TARGET_GROUPS, MIN_SLICE_ROWS, THREADS = 512, 8, 256


def cell_first(c, w, g):
    if c >= g - 1:
        return w
    if w == 1:
        return 0 if c == 0 else 1
    return -(-(c * (w - 1)) // (g - 1))


def slice_count(w, h, gw, gh):
    cells = (gw - 1) * (gh - 1)
    rows_max = min(h, -(-(h - 1) // (gh - 1)) + 1)
    return min(max(1, TARGET_GROUPS // cells), -(-rows_max // MIN_SLICE_ROWS))


def longest_chain(w, h, gw, gh):
    """The most terms one lane of k_bilagrid_backward adds into an accumulator."""
    s = slice_count(w, h, gw, gh)
    cw = max(cell_first(c + 1, w, gw) - cell_first(c, w, gw) for c in range(gw - 1))
    rows = max(cell_first(c + 1, h, gh) - cell_first(c, h, gh) for c in range(gh - 1))
    return -(-(cw * -(-rows // s)) // THREADS)


def workspace_bytes(w, h, shape):
    gw, gh, gl = shape
    up = lambda n: -(-n // 256) * 256
    return up((gw - 1) * (gh - 1) * slice_count(w, h, gw, gh) * 4 * 96 * 8) + up(gl * gh * gw * 12 * 8)


# ---- the frozen fit of tests/test_gpu_bilagrid.py: a smooth image, a smooth target grid, plain Adam on the residual -----
FIT_SIZE, FIT_SHAPE, FIT_STEPS, FIT_LR = (64, 48), (8, 8, 4), 120, 1e-2


def fit_case():
    """(pred [48,64,4] float32, G* [4,8,8,12] float64, target [48,64,4] float64): a seeded smooth premultiplied image
    whose luminance covers (0, 1), and the restatement of a seeded smooth grid applied to it."""
    (w, h), (gw, gh, gl) = FIT_SIZE, FIT_SHAPE
    rng = np.random.default_rng(41)
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / (w - 1), y / (h - 1)
    pred = np.empty((h, w, 4), F)
    for c in range(3):
        a, b, ph = rng.uniform(0.5, 2.0, 2).tolist() + [rng.uniform(0, 6.28)]
        pred[..., c] = 0.5 + 0.45 * np.sin(2 * np.pi * (a * u + b * v) + ph)
    pred[..., 3] = 1.0
    k, j, i = np.mgrid[0:gl, 0:gh, 0:gw]
    G = identity(FIT_SHAPE)
    for m in range(12):
        a, b, c = rng.uniform(-1, 1, 3)
        G[..., m] += 0.15 * np.sin(2.0 * (a * i / (gw - 1) + b * j / (gh - 1) + c * k / (gl - 1)) + m)
    return pred, G, forward(pred, G)[0]


def fit_residual(out, target):
    return float(np.sqrt(np.mean((np.asarray(out, dtype=np.float64)[..., :3] - target[..., :3]) ** 2)))


def fit_reference():
    """The fit in float64 on the host: FIT_STEPS Adam steps at FIT_LR from the identity, tv = 0, driven by
    v_out = (out - target) / npix.  Returns (residual at the start, residual at the end)."""
    pred, _, target = fit_case()
    npix = pred.shape[0] * pred.shape[1]
    G = identity(FIT_SHAPE)
    m1, m2 = np.zeros_like(G), np.zeros_like(G)
    start = fit_residual(forward(pred, G)[0], target)
    for t in range(1, FIT_STEPS + 1):
        v_out = (forward(pred, G)[0] - target) / npix
        grad, _, _ = backward_grid(pred, v_out, FIT_SHAPE)
        G, m1, m2 = adam_step(G, m1, m2, grad, FIT_LR, 0.0, t)
    return start, fit_residual(forward(pred, G)[0], target)
