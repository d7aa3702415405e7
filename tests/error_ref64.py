"""Float64 reference of brush_render_error_scores (brush_amd/csrc/error_score.hip) and its mechanism-based allowance.

The walk is tests/replay_ref.py's (the forward's, rasterize.wgsl:57-101, in float64 on the float32 inputs, with the
float32 values of the constants); this module adds the error map: every pixel carries e = min(max(E, 0), 1) of its
float32 map value E (a NaN counts as 0), and every hit adds fac e to the splat's row, fac = alpha T.

Allowance per hit, from named mechanisms (U = 2^-24):
  fac     d_fac, exactly as replay_ref derives it: fac (rel(alpha) + rel(T) + U), before its calibration factor
  product fac e is one float32 product: e d_fac carried through, plus fac e U for its rounding
  rint    the kernel adds rint(fac e 2^24): half a unit of 2^-24 per hit.
tol_err[g] is the sum over the splat's hits, times C_ERR.  No constant is a fraction of a tensor's maximum.
"""
import numpy as np

from tests.replay_ref import (CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, Q24, T_STOP, U,  # noqa: F401
                              arrays, ratio, tiles, walk32, walk64)

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
    proj, bins, isect, g_from_c = arrays(case)
    err = np.zeros(n)
    tol = np.zeros(n)
    touched = np.zeros(n, bool)
    for tile in tiles(bins, h, w):
        e = e_img[tile.ys, tile.xs]
        for en in walk64(proj, isect, tile):
            g = int(g_from_c[en.c])
            fac = en.alpha if mutate == "ignore_T" else en.alpha * en.T
            d_fac = fac * (en.rel_a + en.relT + U)
            if en.hit.any():
                touched[g] = True
                err[g] += float((fac * e)[en.hit].sum())
                tol[g] += C_ERR * (float((np.abs(e) * d_fac + fac * np.abs(e) * U)[en.hit].sum())
                                   + 0.5 / Q24 * int(en.hit.sum()))
    return dict(err=err, tol_err=tol, touched=touched)


def gate(got_err, ref):
    """The worst err / tol over all splats of a result (float64 [n], view_err / 2^24) against a reference from walk()
    (0 / 0 = 0: a row nobody touched must be exactly zero, any difference there is inf; a NaN anywhere is inf)."""
    return ratio(got_err, ref["err"], ref["tol_err"])


def passes(ratio):
    return ratio <= 1.0


def emulate32(case, error_map):
    """The kernel's arithmetic restated in numpy float32 (replay_ref.walk32: fused multiply-adds through
    float64 with one rounding, exp2 through float64): a stand-in for the device in tests that run anywhere.  Returns
    the per-splat integers (int64 [n])."""
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    e_img = clamp_map(error_map).astype(np.float32)
    proj, bins, isect, g_from_c = arrays(case, np.float32)
    q = np.zeros(n, np.int64)
    for tile in tiles(bins, h, w):
        e = e_img[tile.ys, tile.xs]
        for en in walk32(proj, isect, tile):
            fac = np.where(en.hit, en.alpha * en.T, np.float32(0))
            if en.hit.any():
                q[int(g_from_c[en.c])] += int(np.rint((fac * e).astype(np.float64) * Q24).astype(np.int64).sum())
    return q
