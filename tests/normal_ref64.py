"""References of the normal kernels (brush_amd/csrc/normal_loss.hip: brush_splat_normals, brush_splat_normals_backward,
brush_normal_loss).

ONE statement of the kernels' formulas, in the evaluation order the kernel file's header documents, written over Python
operators (`_splat_formulas`, `_pixel_formulas`) and evaluated three ways:

  * on numpy float32 arrays: every operator is one IEEE float32 operation, so this is the kernels' arithmetic bit for
    bit (the GPU tests hold the kernels to it with array_equal on the bits).  The loss goes through `fixed_sum`, which
    restates the order of the device reduction (per lane over the tiles a workgroup strides over, the xor-shuffle tree,
    the four waves in order, the finalize kernel's rows) in float64;
  * on `Val` pairs (v, e): v the float64 value, e a first-order RUNNING BOUND of the error the float32 evaluation of the
    same expression carries.  Derivation: a float32 operation returns op(a, b) (1 + d), |d| <= U = 2^-24 (round to
    nearest; no underflow at these magnitudes).  With the operands known to |a~ - a| <= e_a, |b~ - b| <= e_b:
        a + b, a - b   e = e_a + e_b + U |a +- b|
        a b            e = |a| e_b + |b| e_a + U |a b|
        a / b          e = (e_a + |a / b| e_b) / |b| + U |a / b|
        sqrt(a)        e = e_a / (2 sqrt a) + U sqrt a
    (products of two errors dropped: first order in U).  Unrolled, e is U times the sum over the expression tree of the
    absolute values of the terms, each weighted by the number of roundings above it: the "U x sum of absolute terms x
    operation depth" form of the other *_ref64 modules, accumulated mechanically instead of by hand.  The float32 inputs
    are exact (e = 0).  No constant is tuned; the piecewise-constant decisions (the counted and valid masks, the axis k
    and the sign s) are taken from the float32 evaluation, as the kernels take them;
  * in torch float64 with the gradients from AUTOGRAD (`loss64`, `splat_normals64`): the mathematics without the
    hand-derived gradient formulas.

A float32 result must lie within e of the float64 autograd value: test_normal_cpu.py checks that of the float32
restatement, which is what the kernels are bitwise equal to.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
TILE, THREADS, WAVE, MAX_ROWS = 16, 256, 64, 1024  # the pixel kernel's launch shape (normal_loss.hip)


# ---------------------------------------------------------------------------- the two number types
class Val:
    """A float64 array with a running bound of its float32 evaluation's error (the module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Val) else Val(x)

    @staticmethod
    def _rounded(v, e):
        return Val(v, e + U * np.abs(v))

    def __add__(self, o):
        o = Val.lift(o)
        return Val._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Val.lift(o)
        return Val._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Val.lift(o)
        return Val._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = Val.lift(o)
        q = self.v / o.v
        return Val._rounded(q, (self.e + np.abs(q) * o.e) / np.abs(o.v))

    def __neg__(self):
        return Val(-self.v, self.e)

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return Val.lift(o) - self

    def __rtruediv__(self, o):
        return Val.lift(o) / self


def _sqrt(x):
    if isinstance(x, Val):
        r = np.sqrt(x.v)
        return Val._rounded(r, x.e / (2.0 * r))
    return np.sqrt(x)


def _where(m, a, b):
    if isinstance(a, Val) or isinstance(b, Val):
        a, b = Val.lift(a), Val.lift(b)
        return Val(np.where(m, a.v, b.v), np.where(m, a.e, b.e))
    return np.where(m, a, b)


def _shift(a, dx, dy):
    """out[y, x] = a[y + dy, x + dx], zero (False) off the frame."""
    if isinstance(a, Val):
        return Val(_shift(a.v, dx, dy), _shift(a.e, dx, dy))
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _c32(x):
    return F(x)


def _cval(x):
    return Val(np.float64(F(x)))  # (the float32 value of the constant, exact)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


# ---------------------------------------------------------------------------- splat normals
def shortest_axis(log_scales):
    """k [N]: the index of the smallest log-scale, the lowest among equals (a NaN never wins)."""
    l = np.asarray(log_scales, F)
    k = np.zeros(l.shape[0], np.int64)
    k = np.where(l[:, 1] < l[:, 0], 1, k)
    lk = l[np.arange(l.shape[0]), k]
    return np.where(l[:, 2] < lk, 2, k)


def _rotmat(q, c):
    """quat_to_rotmat (splat_math.hpp), q = [w, x, y, z] -> R[r][c]."""
    w, x, y, z = q
    x2, y2, z2 = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    one, two = c(1.0), c(2.0)
    return [[one - two * (y2 + z2), two * (xy - wz), two * (xz + wy)],
            [two * (xy + wz), one - two * (x2 + z2), two * (yz - wx)],
            [two * (xz - wy), two * (yz + wx), one - two * (x2 + y2)]]


def _rotmat_vjp(q, vR, c):
    """quat_to_rotmat_vjp (splat_vjp.hpp): G(a, b) = vR[b][a]."""
    w, x, y, z = q
    G = lambda a, b: vR[b][a]
    two, mtwo = c(2.0), c(-2.0)
    return [two * ((x * (G(1, 2) - G(2, 1)) + y * (G(2, 0) - G(0, 2))) + z * (G(0, 1) - G(1, 0))),
            two * ((((mtwo * x) * (G(1, 1) + G(2, 2)) + y * (G(0, 1) + G(1, 0))) + z * (G(0, 2) + G(2, 0))) +
                   w * (G(1, 2) - G(2, 1))),
            two * (((x * (G(0, 1) + G(1, 0)) - (two * y) * (G(0, 0) + G(2, 2))) + z * (G(1, 2) + G(2, 1))) +
                   w * (G(2, 0) - G(0, 2))),
            two * (((x * (G(0, 2) + G(2, 0)) + y * (G(1, 2) + G(2, 1))) - (two * z) * (G(0, 0) + G(1, 1))) +
                   w * (G(0, 1) - G(1, 0)))]


def _splat_formulas(vm, means, quats, k, c, s=None, v_normals=None):
    """vm: the 16 view-matrix words (column-major) as numbers of the type; means [3], quats [4]: lists of [N] arrays of
    the type; k [N] ints.  Returns (n_c [3], dot, v_quats [4] or None); `s` given: the sign to use for the VJP."""
    R = _rotmat(quats, c)
    a = [_where(k == 0, R[r][0], _where(k == 1, R[r][1], R[r][2])) for r in range(3)]
    nc = [(vm[r] * a[0] + vm[4 + r] * a[1]) + vm[8 + r] * a[2] for r in range(3)]
    pc = [((vm[r] * means[0] + vm[4 + r] * means[1]) + vm[8 + r] * means[2]) + vm[12 + r] for r in range(3)]
    d = _dot(nc, pc)
    vq = None
    if v_normals is not None:
        zero = c(0.0)
        va = [s * ((vm[4 * j] * v_normals[0] + vm[4 * j + 1] * v_normals[1]) + vm[4 * j + 2] * v_normals[2])
              for j in range(3)]
        vR = [[_where(k == col, va[r], zero) for col in range(3)] for r in range(3)]
        vq = _rotmat_vjp(quats, vR, c)
    return nc, d, vq


def _cols(a):
    a = np.asarray(a, F)
    return [a[:, j] for j in range(a.shape[1])]


def splat_normals32(viewmat, means, log_scales, quats):
    """The float32 restatement of brush_splat_normals: (normals [N,3] float32, k [N], s [N] float32 = -1 / +1)."""
    vm = [F(x) for x in np.asarray(viewmat, F).reshape(16)]
    k = shortest_axis(log_scales)
    with np.errstate(all="ignore"):
        nc, d, _ = _splat_formulas(vm, _cols(means), _cols(quats), k, _c32)
        s = np.where(d > 0, F(-1.0), F(1.0)).astype(F)
        out = np.stack([s * nc[r] for r in range(3)], axis=1).astype(F)
    return out, k, s


def splat_normals_backward32(viewmat, means, log_scales, quats, v_normals, v_quats):
    """The float32 restatement of brush_splat_normals_backward: v_quats + the VJP (one float32 add per word)."""
    vm = [F(x) for x in np.asarray(viewmat, F).reshape(16)]
    _, k, s = splat_normals32(viewmat, means, log_scales, quats)
    with np.errstate(all="ignore"):
        _, _, vq = _splat_formulas(vm, _cols(means), _cols(quats), k, _c32, s, _cols(v_normals))
        return (np.asarray(v_quats, F) + np.stack(vq, axis=1).astype(F)).astype(F)


def splat_vjp_bound(viewmat, means, log_scales, quats, v_normals):
    """(value [N,4] float64, bound [N,4]) of the VJP's float32 evaluation and the same pair [N,3] of the normals', by
    the running error of the same formulas: (v_quats value, v_quats bound, normals value, normals bound)."""
    vm = [_cval(x) for x in np.asarray(viewmat, F).reshape(16)]
    _, k, s = splat_normals32(viewmat, means, log_scales, quats)
    lift = lambda cols: [Val(np.asarray(x, np.float64)) for x in cols]
    sv = Val(s.astype(np.float64))
    nc, _, vq = _splat_formulas(vm, lift(_cols(means)), lift(_cols(quats)), k, _cval, sv, lift(_cols(v_normals)))
    nc = [sv * x for x in nc]
    st = lambda xs, f: np.stack([getattr(x, f) for x in xs], axis=1)
    return st(vq, "v"), st(vq, "e"), st(nc, "v"), st(nc, "e")


def splat_normals64(viewmat, quats, k, s, v_normals=None):
    """torch float64: s W column k of R(q); with v_normals the gradient of sum(v_normals * normals) with respect to
    the quaternions by AUTOGRAD.  Returns (normals [N,3], v_quats [N,4] or None) as numpy float64."""
    import torch

    vm = torch.as_tensor(np.asarray(viewmat, F).astype(np.float64).reshape(4, 4))  # [c][r]
    W = vm[:3, :3].T
    q = torch.as_tensor(np.asarray(quats, F).astype(np.float64)).requires_grad_(True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    a = R[torch.arange(q.shape[0]), :, torch.as_tensor(np.asarray(k))]
    n = torch.as_tensor(np.asarray(s, np.float64))[:, None] * (a @ W.T)
    if v_normals is None:
        return n.detach().numpy(), None
    g, = torch.autograd.grad((n * torch.as_tensor(np.asarray(v_normals, F).astype(np.float64))).sum(), q)
    return n.detach().numpy(), g.numpy()


# ---------------------------------------------------------------------------- the pixel kernel
def kappa32(weight, w, h):
    return F(np.float64(F(weight)) / np.float64(w * h))


def counted(A, D, alpha_min):
    """The pixels that count, and which rule ruled each other one out (the first that applies)."""
    A, D = np.asarray(A, F), np.asarray(D, F)
    with np.errstate(invalid="ignore"):
        nonfinite = ~(np.isfinite(A) & np.isfinite(D))
        low_alpha = ~nonfinite & ~(A >= F(alpha_min))
        zero_depth = ~nonfinite & ~low_alpha & ~(D > 0)
        counts = (A >= F(alpha_min)) & (D > 0) & (A < np.inf) & (D < np.inf)
    assert np.array_equal(counts, ~(nonfinite | low_alpha | zero_depth))
    return counts, dict(nonfinite=nonfinite, low_alpha=low_alpha, zero_depth=zero_depth)


def _pixel_formulas(A, D, Nr, rx, ry, counts, kappa, c, valid=None):
    """A, D [h,w], Nr: list of three [h,w] or None, rx [1,w], ry [h,1] of the type; counts [h,w] bool; kappa: a number of
    the type.  valid: None (decide it here, float32 only) or the mask to use.  Returns a dict."""
    h, w = counts.shape
    zero = c(0.0)
    z = _where(counts, D / A, zero)
    P = [z * rx, z * ry, z]
    tx = [_shift(p, 1, 0) - _shift(p, -1, 0) for p in P]
    ty = [_shift(p, 0, 1) - _shift(p, 0, -1) for p in P]
    cr = _cross(ty, tx)
    m = _dot(cr, cr)
    ys, xs = np.mgrid[0:h, 0:w]
    pre = ((xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2) & counts & _shift(counts, 1, 0) &
           _shift(counts, -1, 0) & _shift(counts, 0, 1) & _shift(counts, 0, -1))
    if valid is None:
        valid = pre & (m > 0) & (m < np.inf)
    ln = _sqrt(m)
    nd = [_where(valid, x / ln, zero) for x in cr]
    out = dict(pre=pre, valid=valid, nd=nd, m=m)
    if Nr is None:
        return out
    negk = -kappa
    out["l"] = _where(valid, A - _dot(Nr, nd), zero)
    out["v_normals"] = [_where(valid, negk * x, zero) for x in nd]
    vnd = [negk * x for x in Nr]
    d = _dot(nd, vnd)
    vc = [(vnd[i] - nd[i] * d) / ln for i in range(3)]
    vty = [_where(valid, x, zero) for x in _cross(tx, vc)]
    vtx = [_where(valid, x, zero) for x in _cross(vc, ty)]
    vp = [((_shift(vtx[i], -1, 0) - _shift(vtx[i], 1, 0)) + _shift(vty[i], 0, -1)) - _shift(vty[i], 0, 1)
          for i in range(3)]
    vz = (vp[0] * rx + vp[1] * ry) + vp[2]
    out["v_depth"] = _where(counts, vz / A, zero)
    touched = valid | _shift(valid, 1, 0) | _shift(valid, -1, 0) | _shift(valid, 0, 1) | _shift(valid, 0, -1)
    out["touched"] = touched
    out["v_alpha"] = _where(touched, _where(valid, kappa, zero) - (vz * D) / (A * A), zero)
    return out


def _rays(intr, w, h, c, lift):
    fx, fy, cx, cy = (c(x) for x in intr)
    half = c(0.5)
    rx = ((lift(np.arange(w, dtype=F)[None, :]) + half) - cx) / fx
    ry = ((lift(np.arange(h, dtype=F)[:, None]) + half) - cy) / fy
    return rx, ry


def fixed_sum(values, valid):
    """The device reduction of brush_normal_loss in its own order: values [h,w] (float32, read where valid) ->
    (float64 sum, integer count)."""
    h, w = valid.shape
    tx_n, ty_n = -(-w // TILE), -(-h // TILE)
    ntiles = tx_n * ty_n
    G = min(ntiles, MAX_ROWS)
    acc = np.zeros((G, THREADS), np.float64)
    vals = np.where(valid, np.asarray(values, F), F(0.0)).astype(np.float64)
    for t in range(ntiles):  # workgroup t % G takes tile t after its earlier ones; lane = ly * 16 + lx
        x0, y0 = (t % tx_n) * TILE, (t // tx_n) * TILE
        blk = np.zeros((TILE, TILE), np.float64)
        sub = vals[y0:y0 + TILE, x0:x0 + TILE]
        blk[:sub.shape[0], :sub.shape[1]] = sub
        acc[t % G] += blk.reshape(-1)  # (adding +0.0 where nothing is valid changes no bit)

    def tree(v):  # the xor-shuffle tree of a wave: [..., 64] -> [...]
        idx = np.arange(WAVE)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., idx ^ o]
        return v[..., 0]

    def waves(v):  # [..., 256] -> [...]: the tree per wave, the four waves in order
        r = tree(v.reshape(v.shape[:-1] + (THREADS // WAVE, WAVE)))
        return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]

    rows = waves(acc)
    lanes = np.zeros(THREADS, np.float64)
    for r in range(G):  # the finalize kernel: lane t adds rows t, t + 256, ... in that order
        lanes[r % THREADS] += rows[r]
    return float(waves(lanes)), int(valid.sum())


def normal_loss32(intr, pred_alpha, depth, normals_img, weight, alpha_min, v_pred_alpha=None):
    """The float32 restatement of brush_normal_loss.  intr = (fx, fy, cx, cy); pred_alpha, depth [h,w]; normals_img
    [h,w,3] or None (the normals-only form); v_pred_alpha: the alpha channel of v_pred before the call (None: zeros).
    Returns a dict: depth_normals [h,w,3], stats [2] float32, counts / pre / valid / overflow / rule masks, and with
    normals_img: l, v_depth, v_normals_img, v_pred_alpha (after the call), touched."""
    A, D = np.asarray(pred_alpha, F), np.asarray(depth, F)
    h, w = A.shape
    counts, rules = counted(A, D, alpha_min)
    kappa = kappa32(weight, w, h)
    Nr = None if normals_img is None else [np.asarray(normals_img, F)[..., i] for i in range(3)]
    with np.errstate(all="ignore"):
        rx, ry = _rays(intr, w, h, _c32, lambda a: a)
        o = _pixel_formulas(A, D, Nr, rx, ry, counts, kappa, _c32)
        for key in ("nd", "v_normals"):
            if key in o:
                assert all(x.dtype == F for x in o[key])
        res = dict(counts=counts, pre=o["pre"], valid=o["valid"], overflow=o["pre"] & ~(o["m"] < np.inf),
                   degenerate=o["pre"] & (o["m"] == 0), depth_normals=np.stack(o["nd"], axis=2).astype(F), **rules)
        frac = F(np.float64(int(o["valid"].sum())) / np.float64(w * h))
        if Nr is None:
            res["stats"] = np.array([F(0.0), frac], F)
            return res
        s, _ = fixed_sum(o["l"], o["valid"])
        res["stats"] = np.array([F(np.float64(kappa) * s), frac], F)
        base = np.zeros((h, w), F) if v_pred_alpha is None else np.asarray(v_pred_alpha, F)
        res.update(l=o["l"].astype(F), v_depth=o["v_depth"].astype(F),
                   v_normals_img=np.stack(o["v_normals"], axis=2).astype(F), touched=o["touched"],
                   v_pred_alpha=np.where(o["touched"], base + o["v_alpha"], base).astype(F))
    return res


def normal_loss_bound(intr, pred_alpha, depth, normals_img, weight, alpha_min, ref32, depth_err=None):
    """The running error bounds of the float32 evaluation, on the masks of `ref32` (normal_loss32's result): a dict of
    (value float64, bound) pairs for depth_normals, v_depth, v_normals_img, v_alpha, and loss (scalars).  depth_err:
    None (the inputs are exact) or the error [h,w] the given depth already carries against the depth the caller
    compares with (it enters the running bound as the initial error of D)."""
    A, D = np.asarray(pred_alpha, F).astype(np.float64), np.asarray(depth, F).astype(np.float64)
    h, w = A.shape
    counts, valid = ref32["counts"], ref32["valid"]
    # what does not count is never read: give the float64 run harmless numbers there
    A, D = np.where(counts, A, 1.0), np.where(counts, D, 1.0)
    Nr = [Val(np.asarray(normals_img, F)[..., i].astype(np.float64)) for i in range(3)]
    with np.errstate(all="ignore"):
        rx, ry = _rays(intr, w, h, _cval, Val)
        o = _pixel_formulas(Val(A), Val(D, depth_err), Nr, rx, ry, counts, _cval(kappa32(weight, w, h)), _cval,
                            valid=valid)
    stack = lambda xs: (np.stack([x.v for x in xs], axis=2), np.stack([x.e for x in xs], axis=2))
    k = np.float64(kappa32(weight, w, h))
    lv, le = np.where(valid, o["l"].v, 0.0), np.where(valid, o["l"].e, 0.0)
    loss = k * lv.sum()
    # the float64 sum of n terms adds at most n 2^-53 sum|l| (no order assumed); the product and the conversion to
    # float32 one rounding each
    loss_e = k * (le.sum() + valid.sum() * 2.0 ** -53 * np.abs(lv).sum()) + 2.0 * U * abs(loss)
    return dict(depth_normals=stack(o["nd"]), v_normals_img=stack(o["v_normals"]),
                v_depth=(o["v_depth"].v, o["v_depth"].e), v_alpha=(o["v_alpha"].v, o["v_alpha"].e),
                loss=(float(loss), float(loss_e)))


def loss64(intr, pred_alpha, depth, normals_img, weight, counts, valid):
    """torch float64 with AUTOGRAD on the given masks: dict(loss, v_alpha [h,w], v_depth [h,w], v_normals_img [h,w,3],
    depth_normals [h,w,3]) as numpy float64.  kappa is the kernels' float32 value."""
    import torch
    import torch.nn.functional as TF

    fx, fy, cx, cy = (float(F(x)) for x in intr)
    h, w = counts.shape
    cm, vm = torch.as_tensor(counts), torch.as_tensor(valid)
    t64 = lambda a: torch.as_tensor(np.asarray(a, F).astype(np.float64))
    A = torch.where(cm, t64(pred_alpha), torch.ones(())).requires_grad_(True)
    D = torch.where(cm, t64(depth), torch.ones(())).requires_grad_(True)
    Nr = t64(normals_img).requires_grad_(True)
    z = torch.where(cm, D / A, torch.zeros(()))
    rx = ((torch.arange(w, dtype=torch.float64) + 0.5 - cx) / fx)[None, :].expand(h, w)
    ry = ((torch.arange(h, dtype=torch.float64) + 0.5 - cy) / fy)[:, None].expand(h, w)
    P = torch.stack([z * rx, z * ry, z], dim=0)  # [3,h,w]
    Pp = TF.pad(P, (1, 1, 1, 1))
    tx = Pp[:, 1:h + 1, 2:w + 2] - Pp[:, 1:h + 1, 0:w]
    ty = Pp[:, 2:h + 2, 1:w + 1] - Pp[:, 0:h, 1:w + 1]
    c = torch.linalg.cross(ty, tx, dim=0)
    m = torch.where(vm, (c * c).sum(0), torch.ones(()))
    nd = torch.where(vm, c / torch.sqrt(m), torch.zeros(()))  # [3,h,w]
    l = torch.where(vm, A - (Nr.permute(2, 0, 1) * nd).sum(0), torch.zeros(()))
    kappa = float(kappa32(weight, w, h))
    loss = kappa * l.sum()
    gA, gD, gN = torch.autograd.grad(loss, (A, D, Nr))
    return dict(loss=float(loss.detach()), v_alpha=gA.numpy(), v_depth=torch.where(cm, gD, torch.zeros(())).numpy(),
                v_normals_img=gN.numpy(), depth_normals=nd.permute(1, 2, 0).detach().numpy())


# ---------------------------------------------------------------------------- seeded inputs
def intrinsics(w, h):
    """(fx, fy, cx, cy) of a 60-degree-ish pinhole whose centre sits off the pixel grid."""
    f = F(0.9 * max(w, h, 4))
    return (f, F(f * F(1.05)), F(0.5 * w + 0.25), F(0.5 * h - 0.125))


def make_case(w, h, seed=0, bad=True):
    """Seeded inputs of the pixel kernel at w x h: a tilted, rippled surface 3..7 units away under alpha in [0.55, 1],
    a rendered normal map near (0, 0, -1) scaled by alpha, a random v_pred.  bad=True plants, at frames of >= 1000
    pixels, every rule that makes a pixel invalid: alpha below the minimum, D = 0, NaN and +-inf in alpha or D, and 3x3
    blocks 1e12 units away (two such neighbours in different directions make |c|^2 overflow while c stays finite:
    c ~ z^2 times the angle between two neighbouring rays, ~1e24 / f, squared beyond 3.4e38).  At smaller frames with
    bad=True one pixel in eight gets a low alpha or a zero depth.  Returns a dict of float32 arrays and the call's
    weight and alpha_min."""
    rng = np.random.default_rng(7000 + 131 * w + h + seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 5.0 + 1.5 * (xs / max(w - 1, 1) - 0.5) - 1.0 * (ys / max(h - 1, 1) - 0.5) \
        + 0.05 * np.sin(0.9 * xs) * np.cos(0.7 * ys) + rng.uniform(-0.01, 0.01, (h, w))
    A = rng.uniform(0.55, 1.0, (h, w))
    npix = w * h
    if bad and npix >= 1000:
        r = rng.uniform(size=(h, w))
        A[r < 0.02] = rng.uniform(0.0, 0.499, (h, w))[r < 0.02]
        z[(r >= 0.02) & (r < 0.035)] = 0.0
        for lo, val, on_alpha in ((0.035, np.nan, False), (0.04, np.nan, True), (0.045, np.inf, False),
                                  (0.05, np.inf, True), (0.055, -np.inf, False)):
            sel = (r >= lo) & (r < lo + 0.005)
            (A if on_alpha else z)[sel] = val
        for _ in range(max(2, npix // 400)):
            bx, by = int(rng.integers(1, w - 3)), int(rng.integers(1, h - 3))
            z[by:by + 3, bx:bx + 3] = 1e12
    elif bad:
        r = rng.uniform(size=(h, w))
        A[r < 0.06] = 0.3
        z[(r >= 0.06) & (r < 0.125)] = 0.0
    A32 = A.astype(F)
    with np.errstate(invalid="ignore"):
        D32 = (z.astype(F) * A32).astype(F)  # (inf * alpha = inf, nan stays nan; 0 * alpha = 0)
    nr = rng.normal(0.0, 0.3, (h, w, 3))
    nr[..., 2] -= 1.0
    nr = nr / np.linalg.norm(nr, axis=2, keepdims=True) * np.where(np.isfinite(A), A, 0.5)[..., None]
    return dict(w=w, h=h, intr=intrinsics(w, h), alpha=A32, depth=D32, normals_img=nr.astype(F),
                v_pred=rng.normal(0.0, 1.0, (h, w, 4)).astype(F), weight=0.37, alpha_min=0.5)


def make_splats(n, seed=0):
    """Seeded inputs of the splat-normal kernels: a rotated, translated view matrix (column-major, 16 words) and n
    splats in front of and behind the camera, with, when n allows, exact two-way and three-way log-scale ties, a splat
    whose normal is exactly perpendicular to its view ray (dot == 0) and unit quaternions throughout."""
    rng = np.random.default_rng(9000 + n + seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w_, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                  [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                  [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])
    vm = np.zeros((4, 4))  # [c][r]
    vm[:3, :3] = R.T
    vm[3, :3] = rng.uniform(-1, 1, 3)
    vm[3, 3] = 1.0
    means = rng.uniform(-4.0, 4.0, (n, 3)).astype(F)  # both sides of the camera plane
    log_scales = rng.uniform(-3.0, 0.0, (n, 3)).astype(F)
    quats = rng.normal(size=(n, 4))
    quats = (quats / np.linalg.norm(quats, axis=1, keepdims=True)).astype(F)
    viewmat = vm.reshape(16).astype(F)
    if n >= 8:
        log_scales[1] = [-1.0, -2.0, -2.0]   # two-way tie of the smallest: axis 1
        log_scales[2] = [-2.0, -1.0, -2.0]   # two-way tie: axis 0
        log_scales[3] = [-1.5, -1.5, -1.5]   # three-way tie: axis 0
        log_scales[4] = [-1.0, -1.0, -2.0]   # a tie of the larger two: axis 2
        # dot == 0 exactly: identity view, identity rotation, axis 2 = (0, 0, 1), the mean in the plane z = 0
        log_scales[5] = [-1.0, -1.0, -2.0]
    if n >= 8 and seed == -1:  # the identity view, so that row 5's dot is exactly 0
        viewmat = np.eye(4, dtype=F).reshape(16)
        quats[5] = [1.0, 0.0, 0.0, 0.0]
        means[5] = [0.5, -0.25, 0.0]
    return dict(n=n, viewmat=viewmat, means=means, log_scales=log_scales, quats=quats,
                v_normals=rng.normal(size=(n, 3)).astype(F), v_quats0=rng.normal(size=(n, 4)).astype(F))
