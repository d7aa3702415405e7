"""Float64 reference of brush_render_contributions (brush_amd/csrc/contribution.hip) and its mechanism-based allowance.

The walk, its inputs (a `case` dict, tests/contrib_cases.py builds them by hand) and the allowance of sigma, alpha, T
and fac per (pixel, entry) are tests/replay_ref.py's.  Every hit adds fac = alpha T to its splat: the row's max and sum,
and the counts of hits and stops.

Allowance, on top of replay_ref's d_fac = fac (rel(alpha) + rel(T) + U):
  sum     the kernel adds rint(fac 2^24): half a unit of 2^-24 per hit on top.
tol_max[g] is the max over the splat's hits of d_fac (max is 1-Lipschitz), tol_sum[g] their sum; both times C_CONTRIB.
No constant is a fraction of a tensor's maximum.
"""
import numpy as np

from tests.replay_ref import (CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, Q24, T_STOP, U,  # noqa: F401
                              arrays, ratio, tiles, walk32, walk64)

C_CONTRIB = 1.0  # calibration factor of the whole allowance; raised only as far as a measured worst ratio demands

MUTATIONS = ("noclamp", "stop_as_hit", "ignore_T", "last_max")


def walk(case, mutate=None, want_decisions=False):
    """The reference of one case.  Returns a dict of per-splat arrays of case["n"] rows: max, sum (float64), hits,
    stops (int64), tol_max, tol_sum (float64), touched (bool: the splat's row received anything); per pixel alpha
    [h,w] (float64, 1 - T) and last [h,w] (the last added entry's index into isect, 0 if none); and, with
    want_decisions, `decisions`: one distance per alpha test, sigma test and stop test made by a live pixel, in units
    of that entry's allowance (inf where the compared quantity is exact).
    mutate: one of MUTATIONS, a deliberately WRONG reference (the tests check that the gate rejects each)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    proj, bins, isect, g_from_c = arrays(case)
    mx = np.zeros(n)
    sm = np.zeros(n)
    hits = np.zeros(n, np.int64)
    stops = np.zeros(n, np.int64)
    tol_max = np.zeros(n)
    tol_sum = np.zeros(n)
    touched = np.zeros(n, bool)
    alpha_img = np.zeros((h, w))
    last_img = np.zeros((h, w), np.int64)
    decisions = []
    for tile in tiles(bins, h, w):
        last = np.zeros(tile.xs.shape, np.int64)
        for e in walk64(proj, isect, tile, clamp=mutate != "noclamp"):
            g = int(g_from_c[e.c])
            if want_decisions:
                with np.errstate(divide="ignore", invalid="ignore"):
                    da = np.where(e.d_alpha_u > 0, np.abs(e.alpha_u - INV255) / (C_CONTRIB * e.d_alpha_u), np.inf)
                    ds = np.where(e.d_sigma > 0, np.abs(e.sigma) / (C_CONTRIB * e.d_sigma), np.inf)
                    dt = np.abs(e.next_T - T_STOP) / (C_CONTRIB * np.maximum(e.next_T * e.rel_next, 1e-300))
                decisions.append(da[e.live])
                decisions.append(ds[e.live])
                decisions.append(dt[e.passed])
            fac = (e.alpha if mutate == "ignore_T" else e.alpha * e.T)
            d_fac = C_CONTRIB * fac * (e.rel_a + e.relT + U)
            added = e.hit | e.stop if mutate == "stop_as_hit" else e.hit
            if added.any() or e.stop.any():
                touched[g] = True
            if added.any():
                f = fac[added]
                mx[g] = f.flat[-1] if mutate == "last_max" else max(mx[g], float(f.max()))
                sm[g] += float(f.sum())
                hits[g] += int(added.sum())
                tol_max[g] = max(tol_max[g], float(d_fac[added].max()))
                tol_sum[g] += float(d_fac[added].sum()) + 0.5 / Q24 * int(added.sum())
            if mutate != "stop_as_hit":
                stops[g] += int(e.stop.sum())
            last = np.where(e.hit, e.i, last)
        alpha_img[tile.ys, tile.xs] = 1.0 - tile.T
        last_img[tile.ys, tile.xs] = last
    out = dict(max=mx, sum=sm, hits=hits, stops=stops, tol_max=tol_max, tol_sum=tol_sum, touched=touched,
               alpha=alpha_img, last=last_img)
    if want_decisions:
        out["decisions"] = np.concatenate(decisions) if decisions else np.zeros(0)
    return out


def decisions(case):
    """For every alpha test (and the sigma >= 0 test beside it) and every stop test a live pixel makes: the distance
    to its threshold in units of that entry's allowance.  A case is threshold-free when the smallest is above 8."""
    return walk(case, want_decisions=True)["decisions"]


def gate(got, ref):
    """Compares a result (dict of max [n] f32/f64, sum f64, hits, stops) with a reference from walk().
    Returns dict(counts_equal, ratio_max, ratio_sum): the worst err / tol of max and of sum over all splats (0 / 0 = 0:
    a row nobody touched must be exactly zero, any difference there is inf)."""
    counts = bool(np.array_equal(np.asarray(got["hits"], np.int64), ref["hits"]) and
                  np.array_equal(np.asarray(got["stops"], np.int64), ref["stops"]))
    return dict(counts_equal=counts, ratio_max=ratio(got["max"], ref["max"], ref["tol_max"]),
                ratio_sum=ratio(got["sum"], ref["sum"], ref["tol_sum"]))


def passes(g):
    return g["counts_equal"] and g["ratio_max"] <= 1.0 and g["ratio_sum"] <= 1.0


def emulate32(case):
    """The kernel's arithmetic restated in numpy float32 (fused multiply-adds emulated in float64 with one rounding;
    exp2 through float64, so to 0.5 ulp where v_exp_f32 gives 1): a stand-in for the device in tests that run anywhere.
    Returns max (float32), sum (float64 of the q24 integers), hits, stops."""
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    proj, bins, isect, g_from_c = arrays(case, np.float32)
    mx = np.zeros(n, np.float32)
    q = np.zeros(n, np.int64)
    hits = np.zeros(n, np.int64)
    stops = np.zeros(n, np.int64)
    for tile in tiles(bins, h, w):
        for e in walk32(proj, isect, tile):
            g = int(g_from_c[e.c])
            fac = np.where(e.hit, e.alpha * e.T, np.float32(0))
            if e.hit.any():
                mx[g] = max(mx[g], fac.max())
                q[g] += int(np.rint(fac.astype(np.float64) * Q24).astype(np.int64).sum())
                hits[g] += int(e.hit.sum())
            stops[g] += int(e.stop.sum())
    return dict(max=mx, sum=q.astype(np.float64) / Q24, hits=hits, stops=stops)
