"""Float64 reference of brush_render_contributions (brush_amd/csrc/contribution.hip) and its mechanism-based allowance.

The inputs are the kernel's own: the float32 `projected` rows (compact order), the tile lists (`tile_bins`,
`isect` = compact_gid_from_isect) and `g_from_c` = global_from_compact_gid, as a `case` dict (tests/contrib_cases.py
builds them by hand).  For each tile and pixel the walk is the forward's (rasterize.wgsl:57-101), front to back:

    sigma = 0.5 (a dx^2 + c dy^2) + b dx dy,   alpha_u = o exp(-sigma)
    test:  sigma >= 0 and alpha_u >= 1/255     alpha = min(0.999, alpha_u)    next_T = T (1 - alpha)
    next_T <= 1e-4: the pixel ends WITHOUT adding the entry (a `stop` of the splat)
    else: fac = alpha T is added (a `hit`), T = next_T

in float64 on the float32 inputs, with the float32 values of the constants 1/255, 0.999 and 1e-4.

Allowance per (pixel, entry), from named mechanisms (U = 2^-24; every K is a count of float32 roundings):
  sigma   dx = m.x - p.x and dy carry one rounding each; a dx^2 / 2 then sees K_SIG_A = 5 (dx twice, a dx, two fused
          multiply-adds), c dy^2 / 2 sees K_SIG_C = 6 (dy twice, c dy, (c dy) dy, two fma), b dx dy sees K_SIG_B = 5 (dx, dy,
          b dy, (b dy) dx, one fma), each at the magnitude of its own term:  d_sigma = U (5 A + 6 C + 5 B)
  alpha   power = sigma (-log2 e): the constant and the product, K_POW = 2 at sigma; v_exp_f32 to 1 ulp = 2 U; the
          product with o, 1:  rel(alpha) = d_sigma + U (K_POW sigma + K_EXP + 1), carried through exp at slope 1
  T       T' = T (1 - alpha): the error of alpha enters as d_alpha / (1 - alpha), and 1 - alpha and the product round
          once each (K_T = 2):  rel(T') = rel(T) + d_alpha / (1 - alpha) + 2 U, summed over the earlier entries
  fac     alpha T, one product:  d_fac = fac (rel(alpha) + rel(T) + U)
  sum     the kernel adds rint(fac 2^24): half a unit of 2^-24 per hit on top.
tol_max[g] is the max over the splat's hits of d_fac (max is 1-Lipschitz), tol_sum[g] their sum; both times C_CONTRIB.
No constant is a fraction of a tensor's maximum.
"""
import numpy as np

U = 2.0 ** -24
K_SIG_A, K_SIG_C, K_SIG_B = 5.0, 6.0, 5.0
K_POW = 2.0
K_EXP = 2.0   # v_exp_f32: 1 ulp = 2 U
K_T = 2.0
C_CONTRIB = 1.0  # calibration factor of the whole allowance; raised only as far as a measured worst ratio demands

INV255 = float(np.float32(1.0) / np.float32(255.0))
CLAMP = float(np.float32(0.999))
T_STOP = float(np.float32(1e-4))
Q24 = 2.0 ** 24

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
    proj = np.asarray(case["projected"], np.float32).astype(np.float64)
    bins = np.asarray(case["tile_bins"]).astype(np.int64)
    isect = np.asarray(case["isect"]).astype(np.int64)
    g_from_c = np.asarray(case["g_from_c"]).astype(np.int64)
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
    tby, tbx = bins.shape[0], bins.shape[1]
    for ty in range(tby):
        for tx in range(tbx):
            y0, x0 = ty * 16, tx * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, h)), np.arange(x0, min(x0 + 16, w)), indexing="ij")
            pcx, pcy = xs + 0.5, ys + 0.5
            T = np.ones(xs.shape)
            relT = np.zeros(xs.shape)
            live = np.ones(xs.shape, bool)
            last = np.zeros(xs.shape, np.int64)
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
                alpha = alpha_u if mutate == "noclamp" else np.minimum(CLAMP, alpha_u)
                next_T = T * (1.0 - alpha)
                rel_next = relT + d_alpha_u / np.maximum(1.0 - alpha, 1e-300) + K_T * U
                stop = passed & (next_T <= T_STOP)
                hit = passed & ~stop
                if want_decisions:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        da = np.where(d_alpha_u > 0, np.abs(alpha_u - INV255) / (C_CONTRIB * d_alpha_u), np.inf)
                        ds = np.where(d_sigma > 0, np.abs(sigma) / (C_CONTRIB * d_sigma), np.inf)
                        dt = np.abs(next_T - T_STOP) / (C_CONTRIB * np.maximum(next_T * rel_next, 1e-300))
                    decisions.append(da[live])
                    decisions.append(ds[live])
                    decisions.append(dt[passed])
                fac = (alpha if mutate == "ignore_T" else alpha * T)
                d_fac = C_CONTRIB * fac * (rel_a + relT + U)
                added = hit | stop if mutate == "stop_as_hit" else hit
                if added.any() or stop.any():
                    touched[g] = True
                if added.any():
                    f = fac[added]
                    mx[g] = f.flat[-1] if mutate == "last_max" else max(mx[g], float(f.max()))
                    sm[g] += float(f.sum())
                    hits[g] += int(added.sum())
                    tol_max[g] = max(tol_max[g], float(d_fac[added].max()))
                    tol_sum[g] += float(d_fac[added].sum()) + 0.5 / Q24 * int(added.sum())
                if mutate != "stop_as_hit":
                    stops[g] += int(stop.sum())
                T = np.where(hit, next_T, T)
                relT = np.where(hit, rel_next, relT)
                last = np.where(hit, i, last)
                live = live & ~stop
            alpha_img[ys, xs] = 1.0 - T
            last_img[ys, xs] = last
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
    def ratio(err, tol):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / tol)
        return float(np.max(r)) if r.size else 0.0

    counts = bool(np.array_equal(np.asarray(got["hits"], np.int64), ref["hits"]) and
                  np.array_equal(np.asarray(got["stops"], np.int64), ref["stops"]))
    e_max = np.abs(np.asarray(got["max"], np.float64) - ref["max"])
    e_sum = np.abs(np.asarray(got["sum"], np.float64) - ref["sum"])
    return dict(counts_equal=counts, ratio_max=ratio(e_max, ref["tol_max"]), ratio_sum=ratio(e_sum, ref["tol_sum"]))


def passes(g):
    return g["counts_equal"] and g["ratio_max"] <= 1.0 and g["ratio_sum"] <= 1.0


def emulate32(case):
    """The kernel's arithmetic restated in numpy float32 (fused multiply-adds emulated in float64 with one rounding;
    exp2 through float64, so to 0.5 ulp where v_exp_f32 gives 1): a stand-in for the device in tests that run anywhere.
    Returns max (float32), sum (float64 of the q24 integers), hits, stops."""
    f32 = np.float32
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    proj = np.asarray(case["projected"], f32)
    bins = np.asarray(case["tile_bins"]).astype(np.int64)
    isect = np.asarray(case["isect"]).astype(np.int64)
    g_from_c = np.asarray(case["g_from_c"]).astype(np.int64)
    mx = np.zeros(n, f32)
    q = np.zeros(n, np.int64)
    hits = np.zeros(n, np.int64)
    stops = np.zeros(n, np.int64)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    neg_log2e = f32(-1.44269504088896341)
    for ty in range(bins.shape[0]):
        for tx in range(bins.shape[1]):
            y0, x0 = ty * 16, tx * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, h)), np.arange(x0, min(x0 + 16, w)), indexing="ij")
            pcx, pcy = (xs + 0.5).astype(f32), (ys + 0.5).astype(f32)
            T = np.ones(xs.shape, f32)
            live = np.ones(xs.shape, bool)
            for i in range(int(bins[ty, tx, 0]), int(bins[ty, tx, 1])):
                if not live.any():
                    break
                c = int(isect[i])
                g = int(g_from_c[c])
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
                    mx[g] = max(mx[g], fac.max())
                    q[g] += int(np.rint(fac.astype(np.float64) * Q24).astype(np.int64).sum())
                    hits[g] += int(hit.sum())
                stops[g] += int(stop.sum())
                T = np.where(hit, next_T, T)
                live = live & ~stop
    return dict(max=mx, sum=q.astype(np.float64) / Q24, hits=hits, stops=stops)
