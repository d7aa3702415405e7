"""Float64 reference of the depth-distortion replays (brush_amd/csrc/distortion.hip: brush_render_distortion,
brush_distortion_compact_grads) and their mechanism-based allowances.

The walk is tests/replay_ref.py's (the forward's, rasterize.wgsl:57-101, in float64 on the float32 inputs, with the
float32 values of the constants), extended with a per-case `compact_depth` (seeded_depth: non-decreasing along the compact
order, with equal neighbours).  Per pixel, over the hits i = 1..n in list order (entries the forward added):

    w_i = alpha_i T_i,  z_i = compact_depth[cgid_i],  m_i = mu(z_i):  "depth" z;  "ndc" A (1 - near / z) with
    A = far / (far - near) from the float32 near and far,  c_i = m_i - m_first
    L = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 = sum_i w_i (c_i^2 W_{i-1} - 2 c_i M1_{i-1} + M2_{i-1})
    stats = (L, W, M1, M2), the totals of L and of w, w c, w c^2
    g_i = c_i^2 W - 2 c_i M1 + M2,  dL/dm_i = 2 w_i (c_i W - M1),  P_i = sum_{j<=i} w_j g_j
    dL/dalpha_i = T_i g_i - (2 L - P_i) / (1 - alpha_i), 0 where alpha_u > 0.999 (clamped);  vva = vis v(p) dL/dalpha_i
    rows[cgid] (COMPACT id), the seven sums ROW_WORDS = words 0, 1, 2, 3, 4, 8, 9 of the compact gradient row:
      -o sum vva gx, -o sum vva gy, -o/2 sum vva dx^2, -o sum vva dx dy, -o/2 sum vva dy^2, sum vva,
      mu'(z) sum v dL/dm_i         (dx = mean.x - pixel.x, gx = a dx + b dy, gy = b dx + c dy, o the drawn opacity)

Allowances, from named mechanisms only (U = 2^-24; d_fac = fac (rel(alpha) + rel(T) + U) and rel(alpha), rel(T) exactly
as replay_ref derives them, before its calibration factor):
  m       "depth": exact.  "ndc": the kernels carry m~ = -(A near) / z, which differs from m by the constant A: the
          float32 A near (its subtraction, division and product) and the division by z round at the size of
          A near / z:  d_m = 4 U A near / z.
  c       d_c = d_m_i + d_m_first + U |c|.
  stats   the inputs, to first order through the exact partials: sum_i g_i d_fac_i + |dL/dm_i| d_c_i (and the like for
          W, M1, M2); the ROUNDINGS OF THE RUNNING FORM: the k-th hit evaluates g over running sums that carry at most
          k + 1 roundings each and rounds 2 more times itself, all at the magnitude E_k = c^2 W + 2 |c| sum w |c| + M2 of
          the terms it cancels: w_k U (k + 3) E_k; and one rounding per step of each running sum at its own magnitude.
  dalpha  g_i from the TOTALS the forward stored (their stats allowances, through c^2, 2 |c| and 1), d_c through
          |2 c W - 2 M1|, 3 roundings at E_i; P_i: its terms' errors and one rounding per step; THE 2 L - P_i SUBTRACTION
          OVER (1 - alpha_i): (tol(2 L) + tol(P_i) + U |2 L - P_i|) / (1 - alpha_i), the quotient's 2 roundings and the
          error of alpha in 1 - alpha; T_i g_i with rel(T) and the final rounding.  The kernel walks FRONT TO BACK with
          the prefix P_i, so this is the prefix form (no suffix sum).
  vva     vis carries rel(alpha) less the product with o; v dL/dalpha and the product with vis round once each.
  rows    per hit the geometry factor's roundings, K_GEO = 5 at the magnitude of its terms (dx or dy twice, the
          products; gx: its fused multiply-add), plus the summation term (K_TREE + 1 + P) U sum |terms|: 6 levels of the
          wave's tree, the per-record factor, and one rounding per partial sum the float atomics add to the row,
          P = the number of (record, 8x8 quadrant) pairs with a hit.  Word 9 in "ndc": mu' rounds 3 times more.
          A test that pre-fills the rows adds P U |prefill| itself (the atomics round at the row's magnitude).
Each times C_DIST.  No constant is a fraction of a tensor's maximum.
"""
import numpy as np

from tests import contrib_cases as CC
from tests.replay_ref import (CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, T_STOP, U,  # noqa: F401
                              arrays, ratio, tiles, walk64)

C_DIST = 1.0  # calibration factor of every allowance; raised only as far as a measured worst ratio on the GPU demands
K_TREE = 6.0  # levels of the wave64 reduction tree
K_GEO = 5.0   # roundings of a geometry factor (dx^2, dx dy, dy^2, gx, gy) and its product with vva
ROW_WORDS = (0, 1, 2, 3, 4, 8, 9)

MUTATIONS = ("pairs_twice", "ignore_T", "stop_added", "global_row", "no_dmu", "clamp_grad", "suffix_incl")
NDC = dict(mode="ndc", near=0.2, far=50.0)  # the NDC configuration of the tests


def clamped_pair():
    """A faint wide record in front of one with opacity 1.0 centred on the pixel centre (8.5, 8.5), where alpha_u = 1
    clamps to 0.999, and a third behind both: the one pixel where a CLAMPED alpha has a non-zero dL/dalpha (in
    contrib_cases' `clamped` the clamped entries are their pixels' only hits).  The case carries its own depths: the
    front pair must differ."""
    c = CC.make_case("clamped_pair", 16, 16, [(8.0, 8.0, 0.01, 0.0, 0.01, 0.3), (8.5, 8.5, 0.3, 0.0, 0.3, 1.0),
                                              (4.5, 6.5, 0.05, 0.01, 0.05, 0.5)], all_tiles=True)
    c["depth"] = np.array([1.5, 2.25, 2.25], np.float32)
    return c


def all_cases():
    """contrib_cases' and the one case of this module's own."""
    return CC.all_cases() + [clamped_pair()]


def seeded_depth(case, seed=0):
    """float32 [n] compact_depth of a case: non-decreasing along the compact order from a start in [1, 3), every fourth
    step (on average) zero, the others in [0.05, 0.6); entries past num_visible repeat the last.  A case with depths of
    its own (`depth`) keeps them."""
    if "depth" in case:
        return np.asarray(case["depth"], np.float32)
    n = int(case["n"])
    rng = np.random.default_rng(7000 + seed + 13 * n + int(case["w"]))
    steps = np.where(rng.uniform(size=n) < 0.25, 0.0, rng.uniform(0.05, 0.6, n))
    return (rng.uniform(1.0, 3.0) + np.cumsum(steps)).astype(np.float32)


def seeded_v(case, seed=0):
    """float32 [h,w] upstream gradient on L: standard normal."""
    rng = np.random.default_rng(7100 + seed + 7 * int(case["w"]) + int(case["h"]))
    return rng.normal(0.0, 1.0, (int(case["h"]), int(case["w"]))).astype(np.float32)


def scale_a(near, far):
    """A = far / (far - near) of the float32 near and far, in float64."""
    nz, fz = float(np.float32(near)), float(np.float32(far))
    return fz / (fz - nz)


def mu(z, mode="depth", near=0.2, far=None):
    """(m, dm/dz, d_m) of float64 depths z."""
    z = np.asarray(z, np.float64)
    if mode == "depth":
        return z, np.ones_like(z), np.zeros_like(z)
    assert mode == "ndc", mode
    A, nz = scale_a(near, far), float(np.float32(near))
    m = A * (1.0 - nz / z)
    return m, A * nz / (z * z), 4.0 * U * A * nz / np.abs(z)


def walk(case, depth, v=None, mode="depth", near=0.2, far=None, mutate=None):
    """The reference of one case (tests/contrib_cases.py) with compact_depth `depth` [>= num_visible] float32 and the
    upstream gradient v [h,w] float32 (None: zeros).  Returns a dict: stats, tol_stats [h,w,4]; added [h,w] (bool); sum_wg [h,w] (sum_i w_i g_i = 2 L);
    rows, tol_rows, abs_rows [n,7] (by compact id, columns ROW_WORDS; abs_rows: the sum of the |terms|); partials [n]
    (P of the module docstring); touched [n] (bool: the compact id was added to some pixel); risk [n] (the smallest
    distance of one of the record's alpha, sigma, stop or clamp tests at a live pixel to its threshold, in units of that
    test's allowance; a record below 8 may be decided differently in float32).
    mutate: one of MUTATIONS, a deliberately WRONG reference (the tests check that the gate rejects each): pairs_twice
    (ordered pairs: everything doubles), ignore_T (w = alpha), stop_added (the entry that stops a pixel is a hit too),
    global_row (the row of the global id), no_dmu (word 9 without mu'), clamp_grad (a clamped alpha passes its
    gradient), suffix_incl (2 L - P_{i-1}: the suffix sum including i)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    Z = np.asarray(depth, np.float32).astype(np.float64)
    V = np.zeros((h, w)) if v is None else np.asarray(v, np.float32).astype(np.float64)
    assert V.shape == (h, w)
    proj, bins, isect, g_from_c = arrays(case)
    stats, tol_stats = np.zeros((h, w, 4)), np.zeros((h, w, 4))
    sum_wg = np.zeros((h, w))
    added_img = np.zeros((h, w), bool)
    rows, tol_rows, abs_rows = np.zeros((n, 7)), np.zeros((n, 7)), np.zeros((n, 7))
    partials = np.zeros(n)
    touched = np.zeros(n, bool)
    risk = np.full(n, np.inf)
    twice = 2.0 if mutate == "pairs_twice" else 1.0
    for tile in tiles(bins, h, w):
        ys, xs = tile.ys, tile.xs
        quad = ((ys - tile.y0) // 8) * 2 + (xs - tile.x0) // 8
        vt = V[ys, xs]
        recs = []  # the records with an added entry, in list order
        for e in walk64(proj, isect, tile):
            c, a_u, d_a_u = e.c, e.alpha_u, e.d_alpha_u
            added = (e.hit | e.stop) if mutate == "stop_added" else e.hit
            if 0 <= c < n:  # the distance of the record's tests to their thresholds, in allowances
                with np.errstate(divide="ignore", invalid="ignore"):
                    dists = [np.where(d_a_u > 0, np.abs(a_u - INV255) / d_a_u, np.inf)[e.live],
                             np.where(e.d_sigma > 0, np.abs(e.sigma) / e.d_sigma, np.inf)[e.live],
                             (np.abs(e.next_T - T_STOP) / np.maximum(e.next_T * e.rel_next, 1e-300))[e.passed],
                             np.where(d_a_u > 0, np.abs(a_u - CLAMP) / d_a_u, np.inf)[e.passed]]
                risk[c] = min([risk[c]] + [float(x.min()) for x in dists if x.size])
            if added.any():
                fac = np.where(added, e.alpha if mutate == "ignore_T" else e.alpha * e.T, 0.0)
                recs.append(dict(c=c, H=added, w=fac, d_w=np.where(added, fac * (e.rel_a + e.relT + U), 0.0),
                                 alpha=e.alpha, T=e.T, relT=e.relT, rel_a=e.rel_a, vis=e.vis, o=e.o,
                                 d_alpha=np.where(a_u > CLAMP, 0.0, d_a_u),
                                 clamped=(a_u > CLAMP) & (mutate != "clamp_grad"), dx=e.dx, dy=e.dy,
                                 conic=e.conic))
        if not recs:
            continue
        K = len(recs)
        st = lambda key: np.stack([r[key] for r in recs])  # noqa: E731  [K, ph, pw]
        H, W_k, dW_k = st("H"), st("w"), st("d_w")
        cg = np.array([r["c"] for r in recs])
        m_k, dmu_k, d_m_k = mu(Z[cg], mode, near, far)
        first = np.argmax(H, axis=0)  # the first hit of a pixel (0 where it has none: masked by H below)
        m0, d_m0 = m_k[first], d_m_k[first]
        c_k = np.where(H, m_k[:, None, None] - m0[None], 0.0)
        d_c = np.where(H, d_m_k[:, None, None] + d_m0[None] + U * np.abs(c_k), 0.0)
        idx = np.cumsum(H, axis=0) - H  # hits in front of the entry
        wc, wc2, wca = W_k * c_k, W_k * c_k * c_k, W_k * np.abs(c_k)
        Wi, M1i, M2i, M1ai = (np.cumsum(a, axis=0) for a in (W_k, wc, wc2, wca))
        Wx, M1x, M2x, M1ax = Wi - W_k, M1i - wc, M2i - wc2, M1ai - wca
        g_run = c_k * c_k * Wx - 2.0 * c_k * M1x + M2x
        L_run = np.cumsum(W_k * g_run, axis=0)
        L, Wt, M1, M2, M1a = L_run[-1], Wi[-1], M1i[-1], M2i[-1], M1ai[-1]
        # the gradient, from the totals
        g = np.where(H, c_k * c_k * Wt - 2.0 * c_k * M1 + M2, 0.0)
        cwm = np.where(H, c_k * Wt - M1, 0.0)
        dLdm = 2.0 * W_k * cwm
        # ---- allowance of the stats
        E_run = c_k * c_k * Wx + 2.0 * np.abs(c_k) * M1ax + M2x
        n_hits = H.sum(axis=0)
        t_in = lambda gw, gc: (gw * dW_k + gc * d_c).sum(axis=0)  # noqa: E731  the inputs through exact partials
        tol_L = t_in(g, np.abs(dLdm)) + (W_k * U * (idx + 3.0) * E_run).sum(axis=0) + U * np.abs(L_run).sum(axis=0)
        tol_W = dW_k.sum(axis=0) + U * Wi.sum(axis=0)
        tol_M1 = t_in(np.abs(c_k), W_k) + U * (wca.sum(axis=0) + M1ai.sum(axis=0))
        tol_M2 = t_in(c_k * c_k, 2.0 * wca) + U * (2.0 * wc2.sum(axis=0) + M2i.sum(axis=0))
        stats[ys, xs] = np.stack([twice * L, Wt, M1, M2], axis=-1)
        tol_stats[ys, xs] = C_DIST * np.stack([twice * tol_L, tol_W, tol_M1, tol_M2], axis=-1)
        added_img[ys, xs] = n_hits > 0
        # ---- dL/dalpha and its allowance
        alpha, Tk, relT_k, rel_a_k = st("alpha"), st("T"), st("relT"), st("rel_a")
        om = 1.0 - alpha
        E_tot = c_k * c_k * Wt + 2.0 * np.abs(c_k) * M1a + M2
        d_g = np.where(H, c_k * c_k * tol_W + 2.0 * np.abs(c_k) * tol_M1 + tol_M2 + 2.0 * np.abs(cwm) * d_c
                       + 3.0 * U * E_tot, 0.0)
        wg = W_k * g
        P = np.cumsum(wg, axis=0)
        d_P = np.cumsum(g * dW_k + W_k * d_g, axis=0) + U * np.cumsum(np.abs(P), axis=0)
        sum_wg[ys, xs] = P[-1]
        rest = 2.0 * L - (P - wg if mutate == "suffix_incl" else P)
        D = rest / om
        d_D = (2.0 * tol_L + d_P + U * np.abs(rest)) / om + np.abs(D) * (2.0 * U + st("d_alpha") / om)
        dLda = np.where(H & ~st("clamped"), Tk * g - D, 0.0)
        d_dLda = np.where(H & ~st("clamped"), Tk * g * relT_k + Tk * d_g + d_D + U * (np.abs(Tk * g) + np.abs(D)), 0.0)
        vis = st("vis")
        vva = twice * vis * vt[None] * dLda
        d_vva = np.abs(vt)[None] * vis * d_dLda + np.abs(vva) * (rel_a_k + 2.0 * U)
        vm = twice * vt[None] * dLdm  # word 9's terms, before mu'
        d_cwm = np.where(H, np.abs(c_k) * tol_W + Wt * d_c + tol_M1 + U * (np.abs(c_k) * Wt + np.abs(M1)), 0.0)
        d_vm = np.abs(vt)[None] * (2.0 * dW_k * np.abs(cwm) + 2.0 * W_k * d_cwm) + 2.0 * U * np.abs(vm)
        for k, r in enumerate(recs):
            c = r["c"]
            row = c if mutate != "global_row" else int(g_from_c[c])
            if not 0 <= row < n:
                continue
            ca, cb, cc = r["conic"]
            dx, dy, o = r["dx"], r["dy"], r["o"]
            # (geometry factor, the magnitude of the terms it is formed from, the per-record factor)
            geo = ((ca * dx + cb * dy, np.abs(ca * dx) + np.abs(cb * dy), -o),
                   (cb * dx + cc * dy, np.abs(cb * dx) + np.abs(cc * dy), -o),
                   (dx * dx, dx * dx, -0.5 * o), (dx * dy, np.abs(dx * dy), -o), (dy * dy, dy * dy, -0.5 * o),
                   (np.ones_like(dx), np.zeros_like(dx), 1.0))
            Hk = H[k]
            P_k = len(np.unique(quad[Hk]))
            touched[row] = True
            partials[row] += P_k
            for j, (f, fmag, scale) in enumerate(geo):
                rows[row, j] += scale * (vva[k] * f)[Hk].sum()
                abs_rows[row, j] += abs(scale) * np.abs(vva[k] * f)[Hk].sum()
                tol_rows[row, j] += C_DIST * abs(scale) * (d_vva[k] * np.abs(f) + K_GEO * U * np.abs(vva[k]) * fmag)[Hk].sum()
            s9 = 1.0 if mutate == "no_dmu" else dmu_k[k]
            rows[row, 6] += s9 * vm[k][Hk].sum()
            abs_rows[row, 6] += abs(s9) * np.abs(vm[k])[Hk].sum()
            tol_rows[row, 6] += C_DIST * abs(s9) * (d_vm[k] + (3.0 * U if mode == "ndc" else 0.0) * np.abs(vm[k]))[Hk].sum()
    tol_rows += C_DIST * (K_TREE + 1.0 + partials)[:, None] * U * abs_rows
    return dict(stats=stats, tol_stats=tol_stats, added=added_img, sum_wg=sum_wg, rows=rows, tol_rows=tol_rows, abs_rows=abs_rows,
                partials=partials, touched=touched, risk=risk / C_DIST)


def brute_force(case, depth, mode="depth", near=0.2, far=None):
    """L [h,w] as the O(n^2) sum over the unordered pairs of every pixel's hits, in float64, from a walk of its own that
    keeps the (w, m) of every hit: sum_{j<i} w_i w_j (m_i - m_j)^2 with the raw m (no shift).
    Deliberately independent of replay_ref's walk, which the running form is tested against: do not rebuild it on it."""
    w, h = int(case["w"]), int(case["h"])
    Z = np.asarray(depth, np.float32).astype(np.float64)
    proj = np.asarray(case["projected"], np.float32).astype(np.float64)
    bins = np.asarray(case["tile_bins"]).astype(np.int64)
    isect = np.asarray(case["isect"]).astype(np.int64)
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            ty, tx = y // 16, x // 16
            T, ws, ms = 1.0, [], []
            for i in range(int(bins[ty, tx, 0]), int(bins[ty, tx, 1])):
                c = int(isect[i])
                dx, dy = proj[c, 0] - (x + 0.5), proj[c, 1] - (y + 0.5)
                sigma = 0.5 * (proj[c, 2] * dx * dx + proj[c, 4] * dy * dy) + proj[c, 3] * dx * dy
                alpha_u = proj[c, 8] * np.exp(-sigma)
                if sigma < 0.0 or alpha_u < INV255:
                    continue
                alpha = min(CLAMP, alpha_u)
                if T * (1.0 - alpha) <= T_STOP:
                    break
                ws.append(alpha * T)
                ms.append(float(mu(Z[c], mode, near, far)[0]))
                T *= 1.0 - alpha
            acc = 0.0
            for i in range(len(ws)):
                for j in range(i):
                    acc += ws[i] * ws[j] * (ms[i] - ms[j]) ** 2
            out[y, x] = acc
    return out


def gate(ref, stats=None, rows=None, extra_rows_tol=None):
    """Ratios of whichever results are given against a reference from walk(): dict(stats=, rows=).  rows: [n,7] in
    the columns ROW_WORDS.  extra_rows_tol: an allowance of the caller's own on top (a pre-filled row's share)."""
    r = {}
    if stats is not None:
        r["stats"] = ratio(stats, ref["stats"], ref["tol_stats"])
    if rows is not None:
        tol = ref["tol_rows"] if extra_rows_tol is None else ref["tol_rows"] + extra_rows_tol
        r["rows"] = ratio(rows, ref["rows"], tol)
    return r


def passes(r):
    return all(x <= 1.0 for x in r.values())
