"""float64 references of the training half: burn 0.16 Adam::step with the SH-rest lerp and the quaternion chain rule
(adam64), k pending zero-gradient steps of the same rule (replay64), and the loss of train.rs:243-268 with the SSIM of
ssim.rs (loss64).  Each returns, next to the float64 result, a per-element allowance built from named mechanisms, in
the style of the render gate (tests/test_gpu_render.py, the comment above CANDIDATES): every term is a float32 rounding
of the kernel's arithmetic, propagated to the output through the reference's own derivatives, or a threshold whose
side the float32 rounding can change, priced as the jump and counted.  No term is a fraction of a tensor's maximum.

The constants K_* are in units of the float32 unit roundoff U = 2^-24 (or of its ulp, EPS = 2^-23) and are bounds of the
kernels' operation counts; C_ADAM multiplies the Adam allowance's rounding terms, C_SSIM the SSIM roundings of the loss
allowance, each fitted to the worst err/tol measured on an MI355X (profiles/parity_margins.json, sections adam / replay
/ loss / quats).  The Adam worst of 1.0 is set by the half-ulp term of the final subtraction.

`mutate` turns a reference into a wrong one (negative controls: the GPU result must fail the gate against each)."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24          # float32 unit roundoff
EPS = 2.0 ** -23        # float32 ulp of 1
FLT_MIN = float(np.finfo(np.float32).tiny)
DENORM_ULP = 2.0 ** -149

# v_sqrt_f32 on gfx950 with a subnormal argument: measured by
# tests/test_gpu_optimizer_f64.py::test_sqrt_of_subnormal_second_moment.  True: the argument is flushed to zero, which
# the allowance prices with the subnormal term (where v' / bc2 < FLT_MIN only).
SQRT_FLUSHES_SUBNORMAL = True

# ---- Adam -----------------------------------------------------------------------------------------------------------
K_M = 2.0       # m' = fl(fl(b1 m) + fl((1-b1) g)): two products and a sum, all terms of one sign bound |m'|
K_V = 3.0       # v' = fl(fl(b2 v) + fl(fl(g g) (1-b2))): three products and a sum of non-negative terms
K_STEP = 9.0    # x - ((m rbc1) rcp(sqrt(v rbc2) + eps)) lr: v rbc2 (1/2 through the root), v_sqrt_f32 1 ulp, + eps,
                # v_rcp_f32 1 ulp, three products
K_LERP = 1.0    # x fl(1 - l) + st l: the constant 1 - l, two products and a sum, at the scale of x (not of the step)
K_QUAT = 32.0   # v_q / s - q (v_q . q) / s^3 in float32: |q|^2, sqrtf, a division, s^-3 and a 4-term dot (~26 U)
C_ADAM = 1.0    # calibration factor of the whole Adam allowance
CEIL_ADAM = 1e-4  # hard ceiling relative to the step's own terms


def f32(a):
    return np.asarray(a, dtype=np.float32)


def spacing32(a):
    """ulp of the float32 nearest to a (>= the smallest subnormal)."""
    return np.abs(np.spacing(np.abs(f32(a)))).astype(np.float64)


def host_bias_correction_rel(beta: float, t: int) -> float:
    """Relative error bound of the host's float32 rbc = 1 / (1 - powf(beta, t)) (adam_bias_corrections): powf to 1 ulp,
    which the subtraction from 1 turns into ulp(beta^t) / (1 - beta^t) (cancellation at small t), that subtraction's
    own rounding and the division's."""
    p = float(np.float32(beta)) ** t
    return float(spacing32(p)) / (1.0 - p) + 2.0 * U


def adam64(x, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-15, time=1, lerp=None, rest=None, quat_vjp=False,
           dm_in=None, dv_in=None, mutate=None):
    """One step of burn 0.16 Adam::step in float64 on one parameter group.

    x, g, m, v: the float32 arrays exactly as the kernel receives them ([rows, k]); constants given as the float32
    values the kernel is handed.  rest: boolean mask [k] of the SH-rest coefficients that take the lerp
    (train.rs:336-351) when lerp is not None.  quat_vjp: g is the gradient wrt x / |x| (rows of 4), chained to x
    first (gaussian_splats.rs:174-175).  dm_in / dv_in: absolute error bounds already carried by m and v (replay64).

    Returns a dict: x, m, v (float64), tol (allowance of x), tol_m, tol_v, ceil (the hard ceiling of tol), sub (elements
    priced by the subnormal term), terms (the step's own terms)."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    lr, eps = float(np.float32(lr)), float(np.float32(eps))
    x = np.asarray(x, np.float64)
    g = np.asarray(g, np.float64)
    m = np.asarray(m, np.float64)
    v = np.asarray(v, np.float64)
    dm_in = 0.0 if dm_in is None else dm_in
    dv_in = 0.0 if dv_in is None else dv_in
    tq = 0.0
    if quat_vjp and mutate != "no_quat_chain":
        s = np.sqrt(np.sum(x * x, axis=-1, keepdims=True))
        g0 = g
        dot = np.sum(g * x, axis=-1, keepdims=True)
        mag = np.abs(g) / s + np.abs(x) * np.sum(np.abs(g * x), axis=-1, keepdims=True) / s ** 3
        g = g / s - x * dot / s ** 3
        tq = K_QUAT * U * mag   # absolute error of the chained gradient
        # the kernel forms s^-3 = inv_s inv_s inv_s as a float32 of its own: below FLT_MIN (|q| > 4.4e12) it is
        # subnormal or 0, and the term q (v_q . q) s^-3 is lost
        lost = s ** -3.0 < FLT_MIN
        tq = tq + np.where(lost, np.abs(x) * np.sum(np.abs(g0 * x), axis=-1, keepdims=True) / s ** 3, 0.0)
    gmag = np.maximum(np.abs(g), tq / (K_QUAT * U)) if quat_vjp and mutate != "no_quat_chain" else np.abs(g)
    one_b1, one_b2 = 1.0 - b1, 1.0 - b2   # exact in float32 too (Sterbenz)
    A, B = np.abs(b1 * m), one_b1 * np.abs(g)
    m1 = b1 * m + one_b1 * g
    gg = np.abs(g) if mutate == "abs_g" else g * g
    V = b2 * v + one_b2 * gg
    v1 = V
    # moment roundings and what the chained gradient's error does to them; den_m / den_v: a subnormal result's
    # absolute half ulp (the subnormal floor, outside the ceiling)
    den_m, den_v = DENORM_ULP, 2.0 * DENORM_ULP
    dm = K_M * U * (A + B) + den_m + b1 * dm_in + one_b1 * tq
    dv_noq = K_V * U * V + den_v + b2 * dv_in
    # the chained gradient's error tq: through (g + e)^2 - g^2 and the rounding of the kernel's g g, up to (|g| + tq)^2
    dv = dv_noq + one_b2 * (2.0 * np.abs(g) * tq + tq * tq) * (1.0 + K_V * U)
    t = time - 1 if mutate == "bc_tm1" else time
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    rbc1, rbc2 = 1.0 / bc1, 1.0 / bc2
    M = m1 * rbc1
    a = v1 * rbc2
    if mutate == "eps_in_sqrt":
        s2 = np.sqrt(a + eps)
        D = s2
    else:
        s2 = np.sqrt(a)
        D = s2 + eps
    step = lr * M / D
    st = x - step
    # --- allowance, one term per mechanism ---
    t_m = lr * rbc1 * dm / D                                   # rounding of m' through dx/dm
    d = rbc2 * dv
    ds = 2.0 * d / (s2 + np.sqrt(d))                           # |sqrt(a + d) - sqrt(a)| <= min(d / sqrt(a), sqrt(d))
    t_v = np.abs(step) * ds / D                                # rounding of v' through dx/dv
    d0 = rbc2 * (dv - den_v)
    t_den = lr * rbc1 * den_m / D + np.abs(step) * (ds - 2.0 * d0 / (s2 + np.sqrt(d0))) / D  # the subnormal floors' share
    # the quaternion chain rule's share: where v_q / s and q (v_q . q) / s^3 cancel, its float32 error is a large part of
    # the chained gradient, and through v' of the step (Adam normalises by the gradient's own size)
    dq = rbc2 * dv_noq
    t_chain = lr * rbc1 * one_b1 * tq / D + np.abs(step) * (ds - 2.0 * dq / (s2 + np.sqrt(dq))) / D
    t_step = K_STEP * U * np.abs(step)                         # the step expression's own roundings
    r1, r2 = host_bias_correction_rel(beta1, time), host_bias_correction_rel(beta2, time)
    t_rbc = np.abs(step) * (r1 + 0.5 * r2 * s2 / D)            # the host's float32 1 / (1 - powf(beta, t))
    sub = a < FLT_MIN * (1.0 + 1e-6)
    t_sub = np.zeros_like(step)
    if SQRT_FLUSHES_SUBNORMAL:
        # v_sqrt_f32 reads a subnormal argument as 0: the denominator loses sqrt(a) <= sqrt(FLT_MIN) ~ 1.1e-19 next to eps
        t_sub = np.where(sub, lr * np.abs(M) * np.minimum(s2, math.sqrt(FLT_MIN)) / (eps * D), 0.0)
    terms = lr * rbc1 * (A + one_b1 * gmag) / D               # the step's own terms (the chained gradient's for quats)
    tol_st = C_ADAM * (t_m + t_v + t_step) + t_rbc + t_sub
    out = st
    ceil = CEIL_ADAM * terms + C_ADAM * (t_den + t_chain)
    chain = t_chain > CEIL_ADAM * terms
    lerp_mask = None
    if lerp is not None and rest is not None:
        lam = float(np.float32(lerp))
        rest = np.asarray(rest, bool).copy()
        if mutate == "lerp_coef0":
            rest[:] = True
        elif mutate == "no_lerp_coef3" and rest.size > 9:
            rest[9:12] = False
        lerp_mask = np.broadcast_to(rest, st.shape)
        lo = x * (1.0 - lam) + st * lam
        out = np.where(lerp_mask, lo, st)
        t_lerp = K_LERP * U * (2.0 * np.abs(x) * (1.0 - lam) + np.abs(st) * lam + np.abs(lo))
        tol_st = np.where(lerp_mask, lam * (tol_st + 0.5 * spacing32(st)) + C_ADAM * t_lerp, tol_st)
        ceil = np.where(lerp_mask, lam * ceil + 3.0 * U * np.maximum(np.abs(x), np.abs(lo)), ceil)
    half_ulp = 0.5 * spacing32(out)                            # the final float32 subtraction (or lerp sum)
    tol = tol_st + half_ulp
    ceil = ceil + half_ulp
    return dict(x=out, m=m1, v=v1, tol=tol, tol_m=C_ADAM * dm, tol_v=C_ADAM * dv, ceil=ceil, sub=sub & (t_sub > 0),
                chain=np.broadcast_to(chain, tol.shape), terms=terms,
                parts=dict(m=t_m, v=t_v, step=t_step, rbc=t_rbc, sub=t_sub, chain=np.broadcast_to(t_chain, tol.shape),
                           ulp=half_ulp))


def replay64(x, m, v, t0, now, *, lr, beta1=0.9, beta2=0.999, eps=1e-15, lerp=None, rest=None):
    """The pending zero-gradient steps t0+1 .. now of a stored (x, m, v) row block in float64 (t0 per row: [rows, 1]).
    The allowance is the sum of the per-step terms; moment errors carry over from step to step."""
    x = np.asarray(x, np.float64).copy()
    m = np.asarray(m, np.float64).copy()
    v = np.asarray(v, np.float64).copy()
    t0 = np.asarray(t0).reshape(-1, 1)
    tol = np.zeros_like(x)
    dm = np.zeros_like(x)
    dv = np.zeros_like(x)
    sub = np.zeros(x.shape, bool)
    steps = np.zeros(x.shape, np.int64)
    for t in range(int(t0.min()) + 1, now + 1):
        live = np.broadcast_to(t0 < t, x.shape)
        r = adam64(x, np.zeros_like(x), m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, time=t, lerp=lerp, rest=rest,
                   dm_in=dm, dv_in=dv)
        x = np.where(live, r["x"], x)
        m = np.where(live, r["m"], m)
        v = np.where(live, r["v"], v)
        tol = tol + np.where(live, r["tol"], 0.0)
        dm = np.where(live, r["tol_m"], dm)
        dv = np.where(live, r["tol_v"], dv)
        sub |= live & r["sub"]
        steps += live
    return dict(x=x, m=m, v=v, tol=tol, tol_m=dm, tol_v=dv, sub=sub, steps=steps)


def gate(got, want, tol):
    """(worst err/tol, index of that element, number of failing elements); NaN/inf compare by equality."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    err = np.abs(got - want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    err = np.where(same, 0.0, err)
    err = np.where(np.isfinite(err), err, np.inf)
    ratio = err / np.maximum(tol, 1e-300)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i, int((ratio > 1.0).sum())


# ---- loss -----------------------------------------------------------------------------------------------------------
C1, C2 = 0.01 ** 2, 0.03 ** 2
K_BLUR = 1.0     # per blurred value: (4 WIN + 6) U of the blur of |X| (2 WIN fused multiply-adds in the two 1-D passes,
                 # plus the float32 window: expf, a WIN-term sum and a division per weight, once per pass)
K_MAP = 12.0     # the SSIM map and its three derivative maps: two v_rcp_f32 (1 ulp), products, sums, the coefficient
K_BWD = 1.0      # the backward's transposed blur: (4 WIN + 6) U of the transposed blur of |D|, plus the combination
C_SSIM = 0.1     # calibration factor of the SSIM roundings (the K_BLUR / K_MAP / K_BWD terms and the SSIM sums of the loss
                 # value); the L1 coefficient's rounding, the summation of the L1 sums and the clamp's jump are not scaled
# Ceiling, on random [0,1] inputs at 1080p: the allowance is at most 1e-4 of |v_f64| on >= 99.9 % of the elements whose v
# is not a cancellation of its own terms (|v| >= CANCEL_LOSS x res["mag"], the size of the three transposed blurs and the
# L1 sign), and at most 1e-4 of the terms on >= 99.9 % of the rest.  The rest (~9 % of the elements) is out of reach
# relative to |v|: there v = T[d_mu] + 2 a T[d_aa] + b T[d_ab] + L1 sign sums terms of opposite sign to far less than
# each, and every float32 rounding of a term is a rounding of the term's size, not of v's.
CEIL_LOSS = 1e-4
CEIL_LOSS_FRACTION = 0.999
CANCEL_LOSS = 0.1


def window64(win):
    g = np.array([math.exp(-((x - win // 2) ** 2) / (2.0 * 1.5 ** 2)) for x in range(win)], np.float64)
    return g / g.sum()


def gt_as_f32(gt):
    """A u8 target enters as the float32 b / 255, correctly rounded (ld_gt_off); float32 targets as they are."""
    gt = np.asarray(gt)
    if gt.dtype == np.uint8:
        return gt.astype(np.float32) / np.float32(255.0)
    return gt.astype(np.float32)


class _Blur:
    """The 2-D window outer(g, g) with zero padding `pad`, applied as its two 1-D passes (the same linear operator; the
    CPU test checks it against the literal 2-D conv2d of ssim.rs:36-40), and its adjoint."""

    def __init__(self, win, pad, ch):
        import torch

        g = torch.from_numpy(window64(win))
        self.wv = g.reshape(1, 1, win, 1).repeat(ch, 1, 1, 1)
        self.wh = g.reshape(1, 1, 1, win).repeat(ch, 1, 1, 1)
        self.pad, self.ch = pad, ch

    def __call__(self, x):
        import torch.nn.functional as F

        x = F.conv2d(x, self.wv, None, padding=(self.pad, 0), groups=self.ch)
        return F.conv2d(x, self.wh, None, padding=(0, self.pad), groups=self.ch)

    def t(self, y):
        import torch.nn.functional as F

        y = F.conv_transpose2d(y, self.wh, None, padding=(0, self.pad), groups=self.ch)
        return F.conv_transpose2d(y, self.wv, None, padding=(self.pad, 0), groups=self.ch)


def _maps(mx, my, exx, eyy, exy, clamp=True):
    """The SSIM map m and the kernel's three derivative maps (wrt blur(a), blur(a a), blur(a b)) as functions of the five
    blurred moments, in the form k_ssim_forward evaluates them."""
    import torch

    mu_xx, mu_yy, mu_xy = mx * mx, my * my, mx * my
    sxx_raw = exx - mu_xx
    sxx = sxx_raw.clamp_min(0.0) if clamp else sxx_raw
    syy = (eyy - mu_yy).clamp_min(0.0) if clamp else eyy - mu_yy
    sxy = exy - mu_xy
    A1, A2 = 2.0 * mu_xy + C1, 2.0 * sxy + C2
    B1, B2 = mu_xx + mu_yy + C1, sxx + syy + C2
    i1, i2 = 1.0 / B1, 1.0 / B2
    m = A1 * A2 * i1 * i2
    d_eab = 2.0 * A1 * i1 * i2
    d_eaa = -m * i2
    if clamp:
        d_eaa = torch.where(sxx_raw >= 0.0, d_eaa, torch.zeros_like(d_eaa))
    d_mu = 2.0 * my * (A2 - A1) * i1 * i2 - 2.0 * mx * (m * i1) - 2.0 * mx * d_eaa
    mag = dict(m=(A1 * A2 * i1 * i2).abs(), d_eab=d_eab.abs(), d_eaa=d_eaa.abs(),
               d_mu=(2.0 * my * (A2.abs() + A1.abs()) * i1 * i2).abs() + (2.0 * mx * m * i1).abs() + (2.0 * mx * d_eaa).abs())
    return m, d_mu, d_eaa, d_eab, sxx_raw, mag


def loss64(pred, gt, ssim_weight, window=11, grad_scale=1.0, mutate=None, allowance=True):
    """train.rs:243-268 in float64 on the CPU: loss = L1 (1 - w) - SSIM w, alpha in the L1 term only for a 4-channel
    target, the SSIM of ssim.rs (2-D Gaussian window sigma 1.5, zero padding div_ceil(WIN, 2), the (h+2)(w+2) map,
    variances clamped at 0); d loss / d pred (times grad_scale) by autograd.

    pred: [h, w, 4] float32; gt: [h, w, 3|4] float32 or uint8.  Returns a dict: loss, v (d loss / d pred, [h, w, 4]),
    and with `allowance`: tol (per element of v), tol_loss, flips (elements priced by the variance-clamp jump), and the
    fields the allowance was built from."""
    import torch

    pred32 = np.ascontiguousarray(pred, np.float32)
    gt32 = gt_as_f32(gt)
    h, w = pred32.shape[:2]
    gtc = gt32.shape[2]
    win = int(window)
    sw = float(np.float32(ssim_weight))
    gs = float(np.float32(grad_scale))
    p = torch.from_numpy(pred32).double().requires_grad_(True)
    b_all = torch.from_numpy(gt32).double()
    l1_four = gtc == 4 and mutate != "l1_rgb"
    cmp = p if l1_four else p[..., :3]
    l1 = (cmp - (b_all if l1_four else b_all[..., :3])).abs().mean()
    loss = l1
    res = dict()
    if sw > 0.0:
        pad = win // 2 if mutate == "pad_half" else (win + 1) // 2
        blur = _Blur(win, pad, 3)
        a = p[..., :3].permute(2, 0, 1)[None]
        b = b_all[..., :3].permute(2, 0, 1)[None]
        X = [a, b, a * a, b * b, a * b]
        Mo = [blur(t) for t in X]
        m, d_mu, d_eaa, d_eab, sxx_raw, mag = _maps(*Mo, clamp=mutate != "no_clamp")
        ssim = m.mean()
        loss = l1 * (1.0 - sw) + (ssim * sw if mutate == "ssim_sign" else -ssim * sw)
    (loss * gs).backward()
    res["loss"] = float(loss.detach())
    res["v"] = p.grad.numpy()
    if not allowance:
        return res
    u = U
    npix = h * w
    l1_coef = abs((1.0 - sw) * gs / (npix * (4 if l1_four else 3)))
    sign_mag = np.zeros((h, w, 4))
    sign_mag[..., :3] = l1_coef
    if l1_four:
        sign_mag[..., 3] = l1_coef
    # L1: sign(pred - gt) is taken of the same float32 values in kernel and reference (no flip); only its coefficient
    # (1 - w) inv_count grad_scale is rounded
    tol = 4.0 * u * sign_mag
    nflip = 0
    absd = np.abs(pred32.astype(np.float64)[..., :gtc] - gt32.astype(np.float64)) if l1_four else \
        np.abs(pred32.astype(np.float64)[..., :3] - gt32.astype(np.float64)[..., :3])
    sum_l1 = float(absd.sum())
    if sw > 0.0:
        with torch.no_grad():
            kb = K_BLUR * (4 * win + 6) * u
            E = [kb * blur(t.abs()) for t in X]
        Md = [t.detach().clone().requires_grad_(True) for t in Mo]
        outs = _maps(*Md, clamp=mutate != "no_clamp")
        names = ("m", "d_mu", "d_eaa", "d_eab")
        dY = {}
        for j, nm in enumerate(names):
            gr = torch.autograd.grad(outs[j].sum(), Md, retain_graph=j < 3, allow_unused=True)
            dY[nm] = sum((gk.abs() * ek) if gk is not None else 0.0 for gk, ek in zip(gr, E)).detach()
        with torch.no_grad():
            mag = {k: t.detach() for k, t in outs[5].items()}
            mval = outs[0].detach()
            coef = sw * gs / (3.0 * (h + 2) * (w + 2))
            err = {k: dY[k] + K_MAP * u * mag[k] for k in ("d_mu", "d_eaa", "d_eab")}
            jmp = {k: torch.zeros_like(mval) for k in ("d_mu", "d_eaa")}
            flips = torch.zeros_like(mval, dtype=torch.bool)
            if mutate != "no_clamp":
                # the clamp's threshold: sigma_xx within the float32 error of the moments of 0 -> either branch
                mx, exx = Mo[0].detach(), Mo[2].detach()
                dsig = E[2] + 2.0 * mx.abs() * E[0] + 2.0 * u * (exx.abs() + mx * mx)
                flips = sxx_raw.detach().abs() <= dsig
                i2 = 1.0 / ((sxx_raw.detach().clamp_min(0) + (Mo[3].detach() - Mo[1].detach() ** 2).clamp_min(0)) + C2)
                jump = (mval * i2).abs()
                jmp["d_eaa"] = torch.where(flips, jump, torch.zeros_like(jump))
                jmp["d_mu"] = torch.where(flips, 2.0 * mx.abs() * jump, torch.zeros_like(jump))
            nflip = int(flips.sum())
            av, bv = X[0].detach().abs(), X[1].detach().abs()
            kbw = K_BWD * (4 * win + 6) * u
            mag_t = blur.t(mag["d_mu"]) + 2.0 * av * blur.t(mag["d_eaa"]) + bv * blur.t(mag["d_eab"])
            err_t = blur.t(err["d_mu"]) + 2.0 * av * blur.t(err["d_eaa"]) + bv * blur.t(err["d_eab"])
            ts = coef * (err_t + kbw * mag_t + 3.0 * u * mag_t)
            tj = coef * (blur.t(jmp["d_mu"]) + 2.0 * av * blur.t(jmp["d_eaa"]))   # the clamp's jump, priced in full
            res["tol_ssim"] = np.zeros((h, w, 4))
            res["tol_ssim"][..., :3] = ts[0].permute(1, 2, 0).numpy()
            tol[..., :3] += tj[0].permute(1, 2, 0).numpy()
            sign_mag[..., :3] += coef * mag_t[0].permute(1, 2, 0).numpy()
            # loss value: the map values' errors plus the summation (per-lane sequential rows, wave trees, partials)
            seg = 3 * win + 1
            nwave = -(-(w + 2) // (65 - win)) * -(-(h + 2) // seg) * 3
            depth = 2 * seg + 12 + -(-nwave // 64)
            dm_sum = float(dY["m"].sum() + K_MAP * u * mag["m"].sum())
            res["tol_loss_ssim"] = sw / (3.0 * (h + 2) * (w + 2)) * (dm_sum + depth * u * float(mval.abs().sum()))
            t_l1 = (1.0 - sw) / (npix * (4 if l1_four else 3)) * depth * u * sum_l1
            res["tol_loss_fixed"] = t_l1 + 4.0 * u * abs(res["loss"])
            res["flip_mask"] = flips[0].permute(1, 2, 0).numpy()
    else:
        nblk = min(-(-npix // 256), 1024)
        depth = 4 * -(-npix // (nblk * 256)) + 8 + -(-nblk // 64) + 6
        res["tol_loss_fixed"] = depth * u * sum_l1 / (npix * (4 if l1_four else 3)) + 4.0 * u * abs(res["loss"])
    # tol_fixed: what is not scaled by C_SSIM (the L1 coefficient's rounding, the clamp's jump)
    res["tol_fixed"] = tol
    res.setdefault("tol_ssim", np.zeros((h, w, 4)))
    res.setdefault("tol_loss_ssim", 0.0)
    res["tol"] = tol + C_SSIM * res["tol_ssim"]
    res["tol_loss"] = res["tol_loss_fixed"] + C_SSIM * res["tol_loss_ssim"]
    res["mag"] = sign_mag   # the size of v's own terms (the SSIM part's three transposed blurs and the L1 sign)
    res["flips"] = nflip
    return res
