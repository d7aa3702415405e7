"""Float64 reference of brush_render_error_scores (brush_amd/csrc/error_score.hip) and its mechanism-based allowance.

The walk is contrib_ref64.walk's (the forward's, rasterize.wgsl:57-101, in float64 on the float32 inputs, with the
float32 values of the constants), restated here with the error map: every pixel carries e = min(max(E, 0), 1) of its
float32 map value E (a NaN counts as 0), and every hit adds fac e to the splat's row, fac = alpha T.

Allowance per hit, from named mechanisms (U = 2^-24):
  fac     d_fac, exactly as contrib_ref64 derives it: fac (rel(alpha) + rel(T) + U), before its calibration factor
  product fac e is one float32 product: e d_fac carried through, plus fac e U for its rounding
  rint    the kernel adds rint(fac e 2^24): half a unit of 2^-24 per hit.
tol_err[g] is the sum over the splat's hits, times C_ERR.  No constant is a fraction of a tensor's maximum.
"""
import numpy as np

from tests.contrib_ref64 import CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, Q24, T_STOP, U

C_ERR = 1.0  # calibration factor of the whole allowance; raised only as far as a measured worst ratio demands

MUTATIONS = ("ignore_map", "transposed_map", "unclamped", "ignore_T")


def clamp_map(E):
    """e = fminf(fmaxf(E, 0), 1) of a float32 map, as float64: a NaN and the negatives are 0, above 1 is 1."""
    E = np.asarray(E, np.float32).astype(np.float64)
    return np.minimum(np.maximum(np.where(np.isnan(E), 0.0, E), 0.0), 1.0)


def walk(case, error_map, mutate=None):
    """The reference of one case (tests/contrib_cases.py) under `error_map` ([h,w] float32).  Returns a dict of
    per-splat arrays of case["n"] rows: err (float64, the summed fac e), tol_err (float64), touched (bool: the splat was
    added to some pixel).
    mutate: one of MUTATIONS, a deliberately WRONG reference (the tests check that the gate rejects each):
    ignore_map (e = 1), transposed_map (pixel (x, y) reads the map as if it were stored [w,h]: E[x,y]), unclamped (the
    raw map value), ignore_T (fac = alpha)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    E = np.asarray(error_map, np.float32)
    assert E.shape == (h, w), (E.shape, (h, w))
    if mutate == "ignore_map":
        e_img = np.ones((h, w))
    elif mutate == "unclamped":
        e_img = E.astype(np.float64)
    else:
        e_img = clamp_map(E)
    if mutate == "transposed_map":
        e_img = np.ascontiguousarray(e_img.reshape(w, h).T)  # [y, x] <- the word at x h + y
    proj = np.asarray(case["projected"], np.float32).astype(np.float64)
    bins = np.asarray(case["tile_bins"]).astype(np.int64)
    isect = np.asarray(case["isect"]).astype(np.int64)
    g_from_c = np.asarray(case["g_from_c"]).astype(np.int64)
    err = np.zeros(n)
    tol = np.zeros(n)
    touched = np.zeros(n, bool)
    for ty in range(bins.shape[0]):
        for tx in range(bins.shape[1]):
            y0, x0 = ty * 16, tx * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, h)), np.arange(x0, min(x0 + 16, w)), indexing="ij")
            pcx, pcy = xs + 0.5, ys + 0.5
            e = e_img[ys, xs]
            T = np.ones(xs.shape)
            relT = np.zeros(xs.shape)
            live = np.ones(xs.shape, bool)
            for i in range(int(bins[ty, tx, 0]), int(bins[ty, tx, 1])):
                if not live.any():
                    break
                c = int(isect[i])
                g = int(g_from_c[c])
                m_x, m_y, ca, cb, cc = proj[c, 0], proj[c, 1], proj[c, 2], proj[c, 3], proj[c, 4]
                o = proj[c, 8]
                dx, dy = m_x - pcx, m_y - pcy
                A, Cc, B = 0.5 * ca * dx * dx, 0.5 * cc * dy * dy, cb * dx * dy
                sigma = A + Cc + B
                d_sigma = U * (K_SIG_A * np.abs(A) + K_SIG_C * np.abs(Cc) + K_SIG_B * np.abs(B))
                alpha_u = o * np.exp(-sigma)
                rel_a = d_sigma + U * (K_POW * np.abs(sigma) + K_EXP + 1.0)
                d_alpha_u = alpha_u * rel_a
                passed = live & (sigma >= 0.0) & (alpha_u >= INV255)
                alpha = np.minimum(CLAMP, alpha_u)
                next_T = T * (1.0 - alpha)
                rel_next = relT + d_alpha_u / np.maximum(1.0 - alpha, 1e-300) + K_T * U
                stop = passed & (next_T <= T_STOP)
                hit = passed & ~stop
                fac = alpha if mutate == "ignore_T" else alpha * T
                d_fac = fac * (rel_a + relT + U)
                if hit.any():
                    touched[g] = True
                    err[g] += float((fac * e)[hit].sum())
                    tol[g] += C_ERR * (float((np.abs(e) * d_fac + fac * np.abs(e) * U)[hit].sum())
                                       + 0.5 / Q24 * int(hit.sum()))
                T = np.where(hit, next_T, T)
                relT = np.where(hit, rel_next, relT)
                live = live & ~stop
    return dict(err=err, tol_err=tol, touched=touched)


def gate(got_err, ref):
    """The worst err / tol over all splats of a result (float64 [n], view_err / 2^24) against a reference from walk()
    (0 / 0 = 0: a row nobody touched must be exactly zero, any difference there is inf; a NaN anywhere is inf)."""
    d = np.abs(np.asarray(got_err, np.float64) - ref["err"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / ref["tol_err"])
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def passes(ratio):
    return ratio <= 1.0


def emulate32(case, error_map):
    """The kernel's arithmetic restated in numpy float32 (as contrib_ref64.emulate32: fused multiply-adds through
    float64 with one rounding, exp2 through float64): a stand-in for the device in tests that run anywhere.  Returns
    the per-splat integers (int64 [n])."""
    f32 = np.float32
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    e_img = clamp_map(error_map).astype(f32)
    proj = np.asarray(case["projected"], f32)
    bins = np.asarray(case["tile_bins"]).astype(np.int64)
    isect = np.asarray(case["isect"]).astype(np.int64)
    g_from_c = np.asarray(case["g_from_c"]).astype(np.int64)
    q = np.zeros(n, np.int64)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    neg_log2e = f32(-1.44269504088896341)
    for ty in range(bins.shape[0]):
        for tx in range(bins.shape[1]):
            y0, x0 = ty * 16, tx * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, h)), np.arange(x0, min(x0 + 16, w)), indexing="ij")
            pcx, pcy = (xs + 0.5).astype(f32), (ys + 0.5).astype(f32)
            e = e_img[ys, xs]
            T = np.ones(xs.shape, f32)
            live = np.ones(xs.shape, bool)
            for i in range(int(bins[ty, tx, 0]), int(bins[ty, tx, 1])):
                if not live.any():
                    break
                c = int(isect[i])
                p = proj[c]
                dx, dy = p[0] - pcx, p[1] - pcy
                sigma = fma(np.full_like(dx, 0.5), fma(p[2] * dx, dx, (p[4] * dy) * dy), (p[3] * dy) * dx)
                power = sigma * neg_log2e
                alpha_u = p[8] * np.exp2(power.astype(np.float64)).astype(f32)
                passed = live & (power <= 0) & (alpha_u >= f32(1.0) / f32(255.0))
                alpha = np.minimum(f32(0.999), alpha_u)
                next_T = T * (f32(1.0) - alpha)
                stop = passed & (next_T <= f32(1e-4))
                hit = passed & ~stop
                fac = np.where(hit, alpha * T, f32(0))
                if hit.any():
                    q[int(g_from_c[c])] += int(np.rint((fac * e).astype(np.float64) * Q24).astype(np.int64).sum())
                T = np.where(hit, next_T, T)
                live = live & ~stop
    return q
