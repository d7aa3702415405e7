"""Hand-made inputs of brush_render_contributions: the projected rows, tile_bins, compact_gid_from_isect and
global_from_compact_gid are written in numpy, so no projection or sort is involved.  The smallest shapes at which the
kernel can go wrong: the batch boundaries of the 64-record LDS staging, ragged frames, several tiles, a record that
quad_may_pass skips in three quadrants of four, a stack that saturates early, a global-id map with gaps, clamped
opacities, and one seeded random case.

A case is a dict: w, h, n (global splat count), projected [M,9] f32 (compact order: xy, conic a b c, rgb, opacity),
tile_bins [tby,tbx,2] i32, isect [cap] i32 (compact ids, tile after tile, front to back), g_from_c [n] i32 (entries
past M are 0, as the forward leaves them), num_visible = M.

Every case is THRESHOLD-FREE (tests/test_contribution_cpu.py asserts it): no alpha test and no stop test lies within 8
allowances of its threshold, so the GPU must reproduce the reference's counts exactly.  Seeds and opacities (at most 0.9
outside the clamp cases) are chosen for that.
"""
import math

import numpy as np

TILE = 16


def _tiles_of(rec, w, h):
    """Tiles whose pixel-centre box the record can reach with alpha >= 1/255, conservatively (a 0.5 px margin)."""
    mx, my, a, b, c, o = rec
    tbx, tby = -(-w // TILE), -(-h // TILE)
    L = math.log(max(255.0 * min(o, 0.999), 1.0)) + 0.05
    det = a * c - b * b
    ex, ey = math.sqrt(2.0 * L * c / det) + 0.5, math.sqrt(2.0 * L * a / det) + 0.5
    out = []
    for ty in range(tby):
        for tx in range(tbx):
            x0, x1 = tx * TILE + 0.5, min(tx * TILE + TILE, w) - 0.5
            y0, y1 = ty * TILE + 0.5, min(ty * TILE + TILE, h) - 0.5
            if mx + ex >= x0 and mx - ex <= x1 and my + ey >= y0 and my - ey <= y1:
                out.append((ty, tx))
    return out


def make_case(name, w, h, records, n=None, gmap=None, all_tiles=False):
    """records: (mx, my, conic a, b, c, opacity) in depth order, front first; the compact id is the position.
    gmap: global id of every compact id (default: the identity); n: global count (default: max id + 1).
    all_tiles: list every record in every tile instead of the tiles it can reach."""
    m = len(records)
    tbx, tby = -(-w // TILE), -(-h // TILE)
    proj = np.zeros((max(m, 1), 9), np.float32)
    for i, r in enumerate(records):
        proj[i] = [r[0], r[1], r[2], r[3], r[4], 0.25 + 0.5 * ((i * 7) % 3) / 2.0, 0.5, 0.75, r[5]]
    gmap = list(range(m)) if gmap is None else [int(g) for g in gmap]
    assert len(gmap) == m and len(set(gmap)) == m
    n = (max(gmap) + 1 if gmap else 1) if n is None else int(n)
    assert all(0 <= g < n for g in gmap)
    lists = {(ty, tx): [] for ty in range(tby) for tx in range(tbx)}
    for i, r in enumerate(records):
        for t in (lists if all_tiles else _tiles_of(r, w, h)):
            lists[t].append(i)
    bins = np.zeros((tby, tbx, 2), np.int32)
    isect = []
    for ty in range(tby):
        for tx in range(tbx):
            bins[ty, tx, 0] = len(isect)
            isect += lists[(ty, tx)]
            bins[ty, tx, 1] = len(isect)
    g_from_c = np.zeros(n, np.int32)
    g_from_c[:m] = gmap if m <= n else 0
    assert m <= n
    return dict(name=name, w=w, h=h, n=n, projected=proj, tile_bins=bins,
                isect=np.asarray(isect + [0], np.int32),  # (one spare entry: the list is never empty storage)
                num_isect=len(isect), g_from_c=g_from_c, num_visible=m)


def _stack(rng, count, w, h, o_lo, o_hi, s_lo=2.0, s_hi=6.0):
    """`count` random records inside the frame: axis-aligned-ish conics of 1 / s^2 with a mild correlation."""
    recs = []
    for _ in range(count):
        sx, sy = rng.uniform(s_lo, s_hi, 2)
        rho = rng.uniform(-0.5, 0.5)
        a, c = 1.0 / (sx * sx * (1 - rho * rho)), 1.0 / (sy * sy * (1 - rho * rho))
        b = -rho / (sx * sy * (1 - rho * rho))
        recs.append((rng.uniform(0, w), rng.uniform(0, h), a, b, c, rng.uniform(o_lo, o_hi)))
    return recs


def gapped_map(m, seed):
    """A global-id map that is not the identity and has gaps: m distinct ids out of 3 m + 5, shuffled."""
    rng = np.random.default_rng(seed)
    return [int(g) for g in rng.permutation(3 * m + 5)[:m]], 3 * m + 5


def empty():
    return make_case("empty", 16, 16, [], n=4)


def one_record():
    return make_case("one_record", 16, 16, [(8.5, 8.5, 0.05, 0.01, 0.08, 0.7)], n=3, gmap=[2])


def batch(count, seed):
    """`count` faint records in one tile: the list crosses the 64-record batches without saturating."""
    rng = np.random.default_rng(seed)
    gmap, n = gapped_map(count, seed)
    return make_case(f"batch_{count}", 16, 16, _stack(rng, count, 16, 16, 0.02, 0.06, 3.0, 8.0), n=n, gmap=gmap,
                     all_tiles=True)


def ragged():
    """17 x 9: tile 1 holds one column of pixels, its quadrants 1 and 3 lie wholly outside, every quadrant is partial."""
    rng = np.random.default_rng(11)
    recs = _stack(rng, 12, 17, 9, 0.2, 0.9) + [(16.5, 4.5, 0.3, 0.0, 0.3, 0.8)]
    return make_case("ragged_17x9", 17, 9, recs, all_tiles=True)


def four_tiles():
    """2 x 2 tiles with a wide record present in all four, and a few of one tile each."""
    recs = [(16.0, 16.0, 0.004, 0.001, 0.005, 0.6), (5.0, 6.0, 0.2, 0.05, 0.3, 0.85), (27.25, 8.5, 0.1, -0.04, 0.15, 0.5),
            (9.75, 25.0, 0.3, 0.0, 0.2, 0.9), (24.0, 24.5, 0.08, 0.02, 0.06, 0.4)]
    c = make_case("four_tiles", 32, 32, recs, n=9, gmap=[4, 0, 8, 2, 5])
    assert all(int(c["tile_bins"][ty, tx, 1] - c["tile_bins"][ty, tx, 0]) >= 1 for ty in range(2) for tx in range(2))
    return c


def quadrant_skip():
    """A tight splat in the corner of quadrant 0 (reach ~3.1 px): quad_may_pass skips it in the other three quadrants;
    a wide one behind it keeps those waves walking."""
    return make_case("quadrant_skip", 16, 16, [(3.5, 3.5, 1.0, 0.0, 1.0, 0.5), (8.0, 8.0, 0.01, 0.0, 0.01, 0.3)],
                     all_tiles=True)


def saturating():
    """Six flat records of opacity 0.8 take T to 0.2^5 = 3.2e-4; the sixth would take it to 6.4e-5 <= 1e-4 and stops
    every pixel without being added (one stopper per pixel).  100 more records lie behind: two further batches the
    waves must not walk."""
    front = [(8.0, 8.0, 1e-4, 0.0, 1e-4, 0.8)] * 6
    behind = _stack(np.random.default_rng(5), 100, 16, 16, 0.3, 0.9)
    gmap, n = gapped_map(106, 3)
    return make_case("saturating", 16, 16, front + behind, n=n, gmap=gmap, all_tiles=True)


def clamped():
    """Opacity 1.0 centred on a pixel centre: alpha_u = 1 clamps to 0.999 and leaves T = 0.001; the same splat again
    would take T to 1e-6 and stops the pixel.  A third record with opacity 0.9995 clamps too where the first two are
    faint."""
    return make_case("clamped", 16, 16, [(8.5, 8.5, 0.3, 0.0, 0.3, 1.0), (8.5, 8.5, 0.3, 0.0, 0.3, 1.0),
                                         (2.5, 12.5, 0.2, 0.05, 0.2, 0.9995)], all_tiles=True)


def random_case(seed=2):
    """About 200 records on 48 x 32 (3 x 2 tiles), a gapped id map."""
    rng = np.random.default_rng(seed)
    gmap, n = gapped_map(200, seed)
    return make_case("random_200", 48, 32, _stack(rng, 200, 48, 32, 0.05, 0.9, 1.5, 7.0), n=n, gmap=gmap)


# ---- exact in float32 -------------------------------------------------------------------------------------------------
EXACT_O = 0.7


def exact_single():
    """One splat centred on the pixel centre (8.5, 8.5): there sigma = 0, exp2(-0) = 1, T = 1, so fac = o exactly: the
    splat's max has the bits of o."""
    return make_case("exact_single", 16, 16, [(8.5, 8.5, 0.05, 0.01, 0.08, EXACT_O)])


def exact_pair():
    """Two concentric splats of equal conic, o1 = o2 = 0.25: the second's fac = a (1 - a) with a = 0.25 exp(-sigma) grows
    with a below 0.5, so its max sits at the centre: 0.25f * (1.0f - 0.25f), exact."""
    r = (8.5, 8.5, 0.05, 0.01, 0.08, 0.25)
    return make_case("exact_pair", 16, 16, [r, r])


def all_cases():
    return [empty(), one_record(), batch(64, 64), batch(65, 65), batch(129, 129), make_case(
        "frame_16x16", 16, 16, _stack(np.random.default_rng(7), 10, 16, 16, 0.2, 0.9), all_tiles=True),
        ragged(), four_tiles(), quadrant_skip(), saturating(), clamped(), random_case(), exact_single(), exact_pair()]
