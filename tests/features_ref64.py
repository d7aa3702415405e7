"""Float64 reference of the feature replays (brush_amd/csrc/features.hip: brush_render_features,
brush_render_features_backward, brush_render_feature_sums) and their mechanism-based allowances.

The walk is tests/replay_ref.py's (the forward's, rasterize.wgsl:57-101, in float64 on the float32 inputs, with the
float32 values of the constants), extended with C channels: every hit (an entry the forward added, fac = alpha T)

    forward    out[p, c]  += fac f[g, c]                 f [n,C] float32, rows by GLOBAL id
    transpose  grad[g, c] += fac v[p, c]                 v [h,w,C] float32, arbitrary
    sums       q[g, c]    += fac m[p, c]                 m = min(max(M, 0), 1) of a float32 map M (a NaN counts as 0)

Allowances, from named mechanisms only (U = 2^-24; d_fac = fac (rel(alpha) + rel(T) + U) exactly as replay_ref
derives it, before its calibration factor):
  forward    per hit |f| d_fac for the weight, plus |f fac| U for the fused multiply-add's one rounding (the running sum is
             bounded by the sum of the |terms|); summed over the pixel's hits.
  transpose  per hit |v| d_fac + |v fac| U (the product), plus the summation term (6 + P) U sum|fac v| for the row: 6
             levels of the wave's tree, and one rounding per partial sum the float atomics add to the row, P = the number
             of (record, 8x8 quadrant) pairs with a hit (every one sends at most one partial sum per channel).
  sums       per hit |m| d_fac + fac |m| U (the product) + half a unit of 2^-24 (rint), as error_ref64 has it.
Each times C_FEAT.  No constant is a fraction of a tensor's maximum.
"""
import numpy as np

from tests.replay_ref import (CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, Q24, T_STOP, U,  # noqa: F401
                              arrays, fma, ratio, tiles, walk32, walk64)
from tests.error_ref64 import clamp_map

C_FEAT = 1.0  # calibration factor of every allowance; raised only as far as a measured worst ratio demands
K_TREE = 6.0  # levels of the wave64 reduction tree

MUTATIONS = ("chw", "channel_off_by_one", "ignore_T", "stop_added", "compact_row")


def seeded(case, c, seed=0):
    """Seeded inputs of a case at C = c: features [n,c] in [-1, 1], v [h,w,c] normal, maps [h,w,c] in [0, 1] (f32)."""
    rng = np.random.default_rng(4000 + seed + 131 * c + 7 * case["w"] + case["h"] + case["n"])
    f = rng.uniform(-1.0, 1.0, (case["n"], c)).astype(np.float32)
    v = rng.normal(0.0, 1.0, (case["h"], case["w"], c)).astype(np.float32)
    m = rng.uniform(0.0, 1.0, (case["h"], case["w"], c)).astype(np.float32)
    return f, v, m


def one_hot(labels, c):
    """float32 [h,w,c] maps of a uint8 [h,w] label image: channel k is `label == k`; labels >= c give all zeros."""
    return (np.asarray(labels)[..., None] == np.arange(c)[None, None, :]).astype(np.float32)


def _as_chw(a):
    """What a kernel that took the [h,w,C] buffer for [C,h,w] would see at [y, x, c]: the word at (c h + y) w + x."""
    h, w, c = a.shape
    return np.ascontiguousarray(a.reshape(c, h, w).transpose(1, 2, 0))


def walk(case, features, v=None, maps=None, mutate=None):
    """The reference of one case (tests/contrib_cases.py).  features [n,C] float32; v, maps: [h,w,C] float32 or None
    (zeros).  Returns a dict: out, tol_out [h,w,C]; added [h,w] (bool: the pixel received an entry); grad, tol_grad,
    q, tol_q [n,C]; abs_grad [n,C] (sum |fac v|); touched [n] (bool: the splat was added to some pixel); partials [n]
    (P of the module docstring).
    mutate: one of MUTATIONS, a deliberately WRONG reference (the tests check that the gate rejects each): chw (the
    output, v and the maps laid out [C,h,w]), channel_off_by_one (channel c of a row is c + 1, cyclically), ignore_T
    (fac = alpha), stop_added (the entry that stops a pixel is added too), compact_row (the row of the compact id
    instead of the global id)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    F = np.asarray(features, np.float32).astype(np.float64)
    nc = F.shape[1]
    assert F.shape == (n, nc)
    V = np.zeros((h, w, nc)) if v is None else np.asarray(v, np.float32).astype(np.float64)
    M = np.zeros((h, w, nc)) if maps is None else clamp_map(maps)
    assert V.shape == (h, w, nc) and M.shape == (h, w, nc)
    if mutate == "chw":
        V, M = _as_chw(V), _as_chw(M)
    if mutate == "channel_off_by_one":
        F = np.roll(F, -1, axis=1)
    proj, bins, isect, g_from_c = arrays(case)
    out, tol_out = np.zeros((h, w, nc)), np.zeros((h, w, nc))
    added_img = np.zeros((h, w), bool)
    grad, tol_grad, abs_grad = np.zeros((n, nc)), np.zeros((n, nc)), np.zeros((n, nc))
    q, tol_q = np.zeros((n, nc)), np.zeros((n, nc))
    touched = np.zeros(n, bool)
    partials = np.zeros(n)
    for tile in tiles(bins, h, w):
        ys, xs = tile.ys, tile.xs
        quad = ((ys - tile.y0) // 8) * 2 + (xs - tile.x0) // 8
        vt, mt = V[ys, xs], M[ys, xs]
        o_t, tol_t = np.zeros(xs.shape + (nc,)), np.zeros(xs.shape + (nc,))
        any_added = np.zeros(xs.shape, bool)
        for e in walk64(proj, isect, tile):
            g = e.c if mutate == "compact_row" else int(g_from_c[e.c])
            added = (e.hit | e.stop) if mutate == "stop_added" else e.hit
            fac = np.where(added, e.alpha if mutate == "ignore_T" else e.alpha * e.T, 0.0)
            d_fac = np.where(added, fac * (e.rel_a + e.relT + U), 0.0)
            if added.any():
                f = F[g] if g < n else np.zeros(nc)
                fa, dfa = fac[..., None], d_fac[..., None]
                o_t += fa * f
                tol_t += C_FEAT * (np.abs(f) * dfa + np.abs(f) * fa * U)
                any_added |= added
                if g < n:
                    touched[g] = True
                    partials[g] += len(np.unique(quad[added]))
                    grad[g] += (fa * vt).sum(axis=(0, 1))
                    abs_grad[g] += (fa * np.abs(vt)).sum(axis=(0, 1))
                    tol_grad[g] += C_FEAT * (np.abs(vt) * dfa + np.abs(vt) * fa * U).sum(axis=(0, 1))
                    q[g] += (fa * mt).sum(axis=(0, 1))
                    tol_q[g] += C_FEAT * ((mt * dfa + mt * fa * U).sum(axis=(0, 1)) + 0.5 / Q24 * int(added.sum()))
        out[ys, xs], tol_out[ys, xs], added_img[ys, xs] = o_t, tol_t, any_added
    tol_grad += C_FEAT * (K_TREE + partials)[:, None] * U * abs_grad
    if mutate == "chw":
        out, tol_out = _as_chw(out), _as_chw(tol_out)
    if mutate == "channel_off_by_one":
        grad, tol_grad, abs_grad, q, tol_q = (np.roll(a, -1, axis=1) for a in (grad, tol_grad, abs_grad, q, tol_q))
    return dict(out=out, tol_out=tol_out, added=added_img, grad=grad, tol_grad=tol_grad, abs_grad=abs_grad, q=q,
                tol_q=tol_q, touched=touched, partials=partials)


def gate(ref, out=None, grad=None, q=None):
    """Ratios of whichever results are given against a reference from walk(): dict(out=, grad=, q=).  q: the kernel's
    integers over 2^24."""
    r = {}
    if out is not None:
        r["out"] = ratio(out, ref["out"], ref["tol_out"])
    if grad is not None:
        r["grad"] = ratio(grad, ref["grad"], ref["tol_grad"])
    if q is not None:
        r["q"] = ratio(q, ref["q"], ref["tol_q"])
    return r


def passes(r):
    return all(x <= 1.0 for x in r.values())


def emulate32(case, features, v=None, maps=None):
    """The kernels' arithmetic restated in numpy float32 (replay_ref.walk32: fused multiply-adds through
    float64 with one rounding, exp2 through float64): a stand-in for the device in tests that run anywhere.  Returns
    dict(out float32 [h,w,C], grad float32 [n,C] (per record and 8x8 quadrant a float32 sum of the float32 products,
    added to the row in float32: one of the orders the atomics may take), q int64 [n,C])."""
    f32 = np.float32
    w, h, n = int(case["w"]), int(case["h"]), int(case["n"])
    F = np.asarray(features, f32)
    nc = F.shape[1]
    V = np.zeros((h, w, nc), f32) if v is None else np.asarray(v, f32)
    M = np.zeros((h, w, nc), f32) if maps is None else clamp_map(maps).astype(f32)
    proj, bins, isect, g_from_c = arrays(case, f32)
    out = np.zeros((h, w, nc), f32)
    grad = np.zeros((n, nc), f32)
    q = np.zeros((n, nc), np.int64)
    for tile in tiles(bins, h, w):
        ys, xs = tile.ys, tile.xs
        quad = ((ys - tile.y0) // 8) * 2 + (xs - tile.x0) // 8
        vt, mt = V[ys, xs], M[ys, xs]
        acc = np.zeros(xs.shape + (nc,), f32)
        for e in walk32(proj, isect, tile):
            g, hit = int(g_from_c[e.c]), e.hit
            fac = np.where(hit, e.alpha * e.T, f32(0))
            if hit.any():
                fa = fac[..., None]
                acc = np.where(hit[..., None], fma(np.broadcast_to(F[g], acc.shape), np.broadcast_to(fa, acc.shape),
                                                   acc), acc)
                prod = (fa * vt).astype(f32)
                for s in np.unique(quad[hit]):
                    grad[g] = grad[g] + prod[quad == s].sum(axis=0, dtype=f32)
                q[g] += np.rint((fa * mt).astype(f32).astype(np.float64) * Q24).astype(np.int64).sum(axis=(0, 1))
        out[ys, xs] = acc
    return dict(out=out, grad=grad, q=q)
