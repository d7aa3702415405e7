"""numpy restatement of brush_depth_loss (include/brush_hip.h), in two forms.

`reference_f32`: every operation a numpy float32 operation, in exactly the order the header states (numpy's float32
arithmetic is IEEE round-to-nearest and never fused), so the kernel's per-pixel outputs can be compared bit for bit.
`reference_f64`: the same formulas in float64 from the same stored inputs, for comparison with autograd and as the
yardstick of the float32 form.

Per pixel: a = alpha of the render, D = accumulated depth, raw = the target word (uint16 or float32),
t = raw * scale + offset; valid = present(raw) and t > 0 and D > 0 and a >= alpha_min;
  mode "depth"      d = D / a   r = d - t   v_D = g / a          v_a = -(g d) / a
  mode "disparity"  q = a / D   r = q - t   v_D = -(g q) / D     v_a = g / D
g = c sign(r), sign(0) = 0, c = float32(weight / (w h)) formed in float64.
"""
import math

import numpy as np

F = np.float32
MODES = ("depth", "disparity")


def coefficient(weight, npix):
    """c as the entry point forms it: the f32 weight over the pixel count in float64, rounded to f32 once."""
    return F(float(F(weight)) / float(npix))


def present(raw):
    raw = np.asarray(raw)
    if raw.dtype == np.uint16:
        return raw != 0
    assert raw.dtype == np.float32, raw.dtype
    with np.errstate(invalid="ignore"):
        return np.isfinite(raw) & (raw > 0)


def target_f32(raw, scale, offset):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(raw).astype(F) * F(scale) + F(offset)


def valid_f32(alpha, D, raw, scale, offset, alpha_min):
    t = target_f32(raw, scale, offset)
    with np.errstate(invalid="ignore"):
        return present(raw) & (t > 0) & (np.asarray(D, F) > 0) & (np.asarray(alpha, F) >= F(alpha_min))


def reference_f32(alpha, D, raw, *, weight=1.0, scale=1.0, offset=0.0, alpha_min=0.5, mode="depth"):
    """dict(valid [h,w] bool, v_depth, v_alpha [h,w] f32 (0 where invalid), abs_r [h,w] f32 (0 where invalid), c)."""
    assert mode in MODES
    a, D = np.asarray(alpha, F), np.asarray(D, F)
    c = coefficient(weight, a.size)
    t = target_f32(raw, scale, offset)
    valid = valid_f32(a, D, raw, scale, offset, alpha_min)
    v_depth, v_alpha, abs_r = np.zeros(a.shape, F), np.zeros(a.shape, F), np.zeros(a.shape, F)
    av, Dv, tv = a[valid], D[valid], t[valid]
    with np.errstate(all="ignore"):
        if mode == "depth":
            d = Dv / av
            r = d - tv
            g = c * np.sign(r).astype(F)
            v_depth[valid] = g / av
            v_alpha[valid] = -(g * d) / av
        else:
            q = av / Dv
            r = q - tv
            g = c * np.sign(r).astype(F)
            v_depth[valid] = -(g * q) / Dv
            v_alpha[valid] = g / Dv
        abs_r[valid] = np.abs(r)
    assert v_depth.dtype == F and v_alpha.dtype == F and abs_r.dtype == F
    return dict(valid=valid, v_depth=v_depth, v_alpha=v_alpha, abs_r=abs_r, c=c)


def loss_f64(ref):
    """float64(c) times the exactly rounded float64 sum of the f32 |r| words: what stats[0] rounds to f32."""
    return float(ref["c"]) * math.fsum(ref["abs_r"][ref["valid"]].astype(np.float64).tolist())


def valid_fraction(ref):
    """stats[1]: the exact count over the pixel count in float64, rounded to f32 once."""
    return F(float(np.count_nonzero(ref["valid"])) / float(ref["valid"].size))


def reference_f64(alpha, D, raw, *, weight=1.0, scale=1.0, offset=0.0, alpha_min=0.5, mode="depth"):
    """The same from the same stored words in float64 (c, scale, offset and alpha_min as the f32 words the kernel
    receives).  dict(valid, v_depth, v_alpha, abs_r [h,w] f64, c, loss)."""
    assert mode in MODES
    a, D = np.asarray(alpha, F).astype(np.float64), np.asarray(D, F).astype(np.float64)
    c = float(coefficient(weight, a.size))
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(raw).astype(np.float64) * float(F(scale)) + float(F(offset))
        valid = present(raw) & (t > 0) & (D > 0) & (a >= float(F(alpha_min)))
    v_depth, v_alpha, abs_r = np.zeros(a.shape), np.zeros(a.shape), np.zeros(a.shape)
    av, Dv, tv = a[valid], D[valid], t[valid]
    if mode == "depth":
        d = Dv / av
        r = d - tv
        g = c * np.sign(r)
        v_depth[valid] = g / av
        v_alpha[valid] = -(g * d) / av
    else:
        q = av / Dv
        r = q - tv
        g = c * np.sign(r)
        v_depth[valid] = -(g * q) / Dv
        v_alpha[valid] = g / Dv
    abs_r[valid] = np.abs(r)
    return dict(valid=valid, v_depth=v_depth, v_alpha=v_alpha, abs_r=abs_r, c=c,
                loss=c * math.fsum(abs_r[valid].tolist()))


# ---------------------------------------------------------------------------- shared test inputs
def make_case(w, h, gt_dtype, mode, seed, scale, offset):
    """Inputs of one shape for the kernel tests: alpha in [0.05, 1], D / alpha in [0.2, 50] (no denormals anywhere),
    a target that differs from the render by 2 % .. 30 % either way (|r| stays away from 0, so the sign is the same in
    f32 and f64), and every invalidity rule on its own random tenth of the pixels or so: alpha below alpha_min, no
    measurement (raw = 0; f32 also NaN, +inf and negative), t <= 0 through the offset (raw small), D = 0.
    Returns dict(alpha, D, raw, v_pred [h,w,4] f32, alpha_min, rule = {name: mask})."""
    rng = np.random.default_rng(seed)
    n = (h, w)
    alpha_min = 0.35
    alpha = rng.uniform(0.05, 1.0, n).astype(F)
    low = rng.random(n) < 0.15
    alpha[low] = rng.uniform(0.05, 0.349, int(low.sum())).astype(F)
    alpha[~low] = np.maximum(alpha[~low], F(alpha_min))
    dn = np.exp(rng.uniform(math.log(0.2), math.log(50.0), n))          # D / alpha
    D = (dn * alpha).astype(F)
    ratio = rng.uniform(0.02, 0.3, n) * rng.choice([-1.0, 1.0], n)      # target = rendered * (1 + ratio)
    want_t = (dn if mode == "depth" else 1.0 / dn) * (1.0 + ratio)      # in loss space
    # raw such that raw * scale + offset = want_t; u16 needs raw in 1..65535 (the caller picks scale to fit)
    raw64 = (want_t - offset) / scale
    if gt_dtype == np.uint16:
        raw = np.clip(np.round(raw64), 1, 65535).astype(np.uint16)
    else:
        raw = raw64.astype(F)
    rule = {"alpha": low}
    pick = lambda p: rng.random(n) < p
    m = pick(0.1)
    raw[m] = 0
    rule["absent"] = m
    if gt_dtype == np.float32:
        for name, val in (("nan", np.nan), ("inf", np.inf), ("negative", -1.5)):
            m = pick(0.04)
            raw[m] = val
            rule[name] = m
    if offset < 0:  # a present target that the offset takes to t <= 0
        m = pick(0.08)
        small = F(-offset / scale * 0.5)
        raw[m] = max(int(small), 1) if gt_dtype == np.uint16 else small
        rule["t<=0"] = m
    m = pick(0.1)
    D[m] = 0.0
    rule["D=0"] = m
    v_pred = rng.standard_normal((h, w, 4)).astype(F)
    return dict(alpha=alpha, D=D, raw=raw, v_pred=v_pred, alpha_min=alpha_min, rule=rule)
