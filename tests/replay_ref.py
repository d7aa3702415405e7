"""The compositing-replay walk of the references: the Python counterpart of brush_amd/csrc/replay_walk.hpp.

The five replay kernels share one walk on the device; their references (contrib_ref64, error_ref64, median_ref64,
features_ref64, distortion_ref64) share this one, and each keeps only what its feature does with a hit.  The inputs are
the kernels' own: the float32 `projected` rows (compact order), the tile lists (`tile_bins`, `isect` =
compact_gid_from_isect) and `g_from_c` = global_from_compact_gid, as a `case` dict (tests/contrib_cases.py builds them
by hand).  For each tile and pixel the walk is the forward's (rasterize.wgsl:57-101), front to back:

    sigma = 0.5 (a dx^2 + c dy^2) + b dx dy,   alpha_u = o exp(-sigma)
    test:  sigma >= 0 and alpha_u >= 1/255     alpha = min(0.999, alpha_u)    next_T = T (1 - alpha)
    next_T <= 1e-4: the pixel ends WITHOUT adding the entry (a `stop` of the splat)
    else: fac = alpha T is added (a `hit`), T = next_T

walk64 does it in float64 on the float32 inputs, with the float32 values of the constants 1/255, 0.999 and 1e-4, and
carries the allowance beside the values; walk32 restates the kernels' float32 arithmetic.

Allowance per (pixel, entry), from named mechanisms (U = 2^-24; every K is a count of float32 roundings):
  sigma   dx = m.x - p.x and dy carry one rounding each; a dx^2 / 2 then sees K_SIG_A = 5 (dx twice, a dx, two fused
          multiply-adds), c dy^2 / 2 sees K_SIG_C = 6 (dy twice, c dy, (c dy) dy, two fma), b dx dy sees K_SIG_B = 5 (dx, dy,
          b dy, (b dy) dx, one fma), each at the magnitude of its own term:  d_sigma = U (5 A + 6 C + 5 B)
  alpha   power = sigma (-log2 e): the constant and the product, K_POW = 2 at sigma; v_exp_f32 to 1 ulp = 2 U; the
          product with o, 1:  rel(alpha) = d_sigma + U (K_POW sigma + K_EXP + 1), carried through exp at slope 1
  T       T' = T (1 - alpha): the error of alpha enters as d_alpha / (1 - alpha), and 1 - alpha and the product round
          once each (K_T = 2):  rel(T') = rel(T) + d_alpha / (1 - alpha) + 2 U, summed over the earlier entries
  fac     alpha T, one product:  d_fac = fac (rel(alpha) + rel(T) + U)
The walk hands out rel(alpha) and rel(T); d_fac and everything behind it belong to the feature, with its own
calibration factor.  No constant is a fraction of a tensor's maximum.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
K_SIG_A, K_SIG_C, K_SIG_B = 5.0, 6.0, 5.0
K_POW = 2.0
K_EXP = 2.0   # v_exp_f32: 1 ulp = 2 U
K_T = 2.0

INV255 = float(np.float32(1.0) / np.float32(255.0))
CLAMP = float(np.float32(0.999))
T_STOP = float(np.float32(1e-4))
Q24 = 2.0 ** 24


def arrays(case, dtype=np.float64):
    """(projected, tile_bins, isect, g_from_c) of a case: the float32 rows as `dtype` (np.float64: every float32 value
    exactly; np.float32: as they are), the indices as int64."""
    return (np.asarray(case["projected"], np.float32).astype(dtype, copy=False),
            np.asarray(case["tile_bins"]).astype(np.int64), np.asarray(case["isect"]).astype(np.int64),
            np.asarray(case["g_from_c"]).astype(np.int64))


def tiles(bins, h, w):
    """Every 16x16 tile of an h x w frame, row-major: ty, tx, y0, x0, the pixel index blocks ys, xs (ragged at the
    right and bottom edges) and the tile's list range [r0, r1) in isect."""
    for ty in range(bins.shape[0]):
        for tx in range(bins.shape[1]):
            y0, x0 = ty * 16, tx * 16
            ys, xs = np.meshgrid(np.arange(y0, min(y0 + 16, h)), np.arange(x0, min(x0 + 16, w)), indexing="ij")
            yield SimpleNamespace(ty=ty, tx=tx, y0=y0, x0=x0, ys=ys, xs=xs, r0=int(bins[ty, tx, 0]),
                                  r1=int(bins[ty, tx, 1]))


def walk64(proj, isect, tile, clamp=True):
    """The float64 walk of one tile (proj, isect from arrays(case); tile from tiles()).  Yields one record per list
    entry while a pixel is live, every field but the scalars a [ph, pw] block: i (the position in isect), c (compact id),
    conic (a, b, c), o, dx, dy, sigma, d_sigma, vis = exp(-sigma), alpha_u, rel_a = rel(alpha), d_alpha_u, alpha,
    next_T, rel_next = rel(next_T), passed (live and through the sigma and alpha tests), stop, hit, and the state BEFORE
    the entry: T, relT = rel(T), live.  The state moves on after the consumer's body has run; its arrays are replaced,
    never written in place, so a consumer may keep them.  When the walk ends it leaves the final T in tile.T.
    clamp=False: alpha = alpha_u (a deliberately WRONG walk, contrib_ref64's `noclamp`)."""
    pcx, pcy = tile.xs + 0.5, tile.ys + 0.5
    T = np.ones(tile.xs.shape)
    relT = np.zeros(tile.xs.shape)
    live = np.ones(tile.xs.shape, bool)
    for i in range(tile.r0, tile.r1):
        if not live.any():
            break
        c = int(isect[i])
        m_x, m_y, ca, cb, cc = proj[c, 0], proj[c, 1], proj[c, 2], proj[c, 3], proj[c, 4]
        o = proj[c, 8]
        dx, dy = m_x - pcx, m_y - pcy
        A, Cc, B = 0.5 * ca * dx * dx, 0.5 * cc * dy * dy, cb * dx * dy
        sigma = A + Cc + B
        d_sigma = U * (K_SIG_A * np.abs(A) + K_SIG_C * np.abs(Cc) + K_SIG_B * np.abs(B))
        vis = np.exp(-sigma)
        alpha_u = o * vis
        rel_a = d_sigma + U * (K_POW * np.abs(sigma) + K_EXP + 1.0)
        d_alpha_u = alpha_u * rel_a
        passed = live & (sigma >= 0.0) & (alpha_u >= INV255)
        alpha = np.minimum(CLAMP, alpha_u) if clamp else alpha_u
        next_T = T * (1.0 - alpha)
        rel_next = relT + d_alpha_u / np.maximum(1.0 - alpha, 1e-300) + K_T * U
        stop = passed & (next_T <= T_STOP)
        hit = passed & ~stop
        yield SimpleNamespace(i=i, c=c, conic=(ca, cb, cc), o=o, dx=dx, dy=dy, sigma=sigma, d_sigma=d_sigma, vis=vis,
                              alpha_u=alpha_u, rel_a=rel_a, d_alpha_u=d_alpha_u, alpha=alpha, next_T=next_T,
                              rel_next=rel_next, passed=passed, stop=stop, hit=hit, T=T, relT=relT, live=live)
        T = np.where(hit, next_T, T)
        relT = np.where(hit, rel_next, relT)
        live = live & ~stop
    tile.T = T


def fma(a, b, c):
    """A float32 fused multiply-add: through float64 (the product of two float32 is exact there) with one rounding."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def walk32(proj, isect, tile):
    """The kernels' walk of one tile restated in numpy float32 (proj, isect from arrays(case, np.float32)): fused
    multiply-adds through float64 with one rounding; exp2 through float64, so to 0.5 ulp where v_exp_f32 gives 1.
    Yields per list entry, while a pixel is live: i, c, p (the entry's float32 row), dx, dy, sigma, power, alpha_u,
    alpha, next_T, passed, stop, hit and the state BEFORE the entry (T, live); the state moves on after the consumer's
    body has run."""
    f32 = np.float32
    neg_log2e = f32(-1.44269504088896341)
    pcx, pcy = (tile.xs + 0.5).astype(f32), (tile.ys + 0.5).astype(f32)
    T = np.ones(tile.xs.shape, f32)
    live = np.ones(tile.xs.shape, bool)
    for i in range(tile.r0, tile.r1):
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
        yield SimpleNamespace(i=i, c=c, p=p, dx=dx, dy=dy, sigma=sigma, power=power, alpha_u=alpha_u, alpha=alpha,
                              next_T=next_T, passed=passed, stop=stop, hit=hit, T=T, live=live)
        T = np.where(hit, next_T, T)
        live = live & ~stop


def ratio(got, want, tol):
    """The worst |got - want| / tol (0 / 0 = 0: where the allowance is zero the value must be exact, any difference
    there is inf; a NaN anywhere is inf)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0
