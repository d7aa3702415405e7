"""Hand-made inputs of brush_render_median_depth: the cases of tests/contrib_cases.py with a camera-space z per compact id,
plus directed cases for what only the median pick can get wrong: an exact tie at the level (`<=`, not `<`), a crossing on
either side of a 64-record staging batch, and a pixel that stops before it ever crosses (level 0.95 only; see
stop_before_crossing).  Also the small rendered scene the GPU test and its CPU twin share.

A case is a contrib_cases dict with one more entry: z [max(n, 1)] f32, indexed by compact id as brush_render_forward_depth
leaves compact_depth (entries past num_visible are never read; here they hold a NaN).  Every z is distinct, so a depth
identifies its entry.
"""
import numpy as np

from tests import contrib_cases as CC

LEVELS = (0.25, 0.5, 0.75)
STOP_LEVEL = 0.95  # the level of stop_before_crossing


def with_z(case):
    """The case with z[c] = 1 + 0.37 c for every compact id c (float32, distinct, increasing with the list order)."""
    m, n = int(case["num_visible"]), max(int(case["n"]), 1)
    z = np.full(n, np.nan, np.float32)
    z[:m] = (1.0 + 0.37 * np.arange(m)).astype(np.float32)
    return dict(case, z=z)


EXACT_HALF_REC = (8.5, 8.5, 0.05, 0.01, 0.08)


def exact_half(first_opacity=0.5):
    """Two concentric records, opacities 0.5 and 0.3, on 16 x 16.  At pixel (8, 8) sigma = 0, exp2(-0) = 1 and T = 1, so
    next_T = 1 - 0.5 = 0.5 exactly: at level 0.5 record 0 is the median there under `<=`, record 1 under `<`.  With the
    first opacity one ulp below 0.5 next_T is just above 0.5 and record 1 is the median."""
    return with_z(CC.make_case("exact_half", 16, 16, [EXACT_HALF_REC + (float(first_opacity),),
                                                      EXACT_HALF_REC + (0.3,)]))


def exact_half_below():
    c = exact_half(float(np.nextafter(np.float32(0.5), np.float32(0.0))))
    c["name"] = "exact_half_below"
    return c


def cross_at(position):
    """`position` - 1 flat records of opacity 0.005 (T falls to ~0.73), then one of 0.6 that takes every pixel to ~0.29,
    then 20 random records behind, listed in every tile.  At level 0.5 the 0.6 record is every pixel's median: with
    position = 64 the last entry of the first staging batch, with 65 the first of the second.  (Level 0.25 is crossed
    by the 58th flat record, level 0.75 among the records behind.)"""
    flat = [(8.0, 8.0, 1e-4, 0.0, 1e-4, 0.005)] * (position - 1)
    cross = [(8.0, 8.0, 1e-4, 0.0, 1e-4, 0.6)]
    behind = CC._stack(np.random.default_rng(position), 20, 16, 16, 0.3, 0.9)
    gmap, n = CC.gapped_map(position + 20, position)
    return with_z(CC.make_case(f"cross_at_{position}", 16, 16, flat + cross + behind, n=n, gmap=gmap, all_tiles=True))


def stop_before_crossing():
    """For level 0.95 (t_level = 0.05) ONLY.  A stopping entry can precede the crossing only when T > t_level and
    T (1 - alpha) <= 1e-4 with alpha <= 0.999, i.e. t_level < 0.1: never at the levels 0.25 / 0.5 / 0.75, so the wrong
    reference that counts a stopping entry needs this case.  A flat record of opacity 0.92 leaves T = 0.08 > 0.05; a flat
    record of opacity 1 then stops the pixels within ~5 px of (8, 8) (alpha >= 0.99875) without being added: those have
    no median.  Further out it is added and crosses.  A third record behind would cross if the walk went on."""
    recs = [(8.0, 8.0, 1e-4, 0.0, 1e-4, 0.92), (8.0, 8.0, 1e-4, 0.0, 1e-4, 1.0), (8.0, 8.0, 0.01, 0.0, 0.01, 0.6)]
    return with_z(CC.make_case("stop_before_crossing", 16, 16, recs, n=7, gmap=[5, 1, 3], all_tiles=True))


def new_cases():
    return [exact_half(), exact_half_below(), cross_at(64), cross_at(65)]


def all_cases():
    """Every (case, levels): the contribution cases and the new ones at LEVELS, stop_before_crossing at STOP_LEVEL."""
    return [(with_z(c), LEVELS) for c in CC.all_cases()] + [(c, LEVELS) for c in new_cases()] + \
        [(stop_before_crossing(), (STOP_LEVEL,))]


def case_level_params():
    return [(c, lv) for c, levels in all_cases() for lv in levels]


def param_id(p):
    return f"{p[0]['name']}-{p[1]:g}"


# ---------------------------------------------------------------------------- the rendered scene
SCENE_N = 300


def rendered_scene(seed=17):
    """A few hundred splats in front of the reference test camera ((0, 0, -8), looking down +z): a mix of faint and
    nearly opaque ones at depths 4..12 from the camera, SH degree 0.  Returns the five parameter arrays (float32; unit
    quaternions), as Splats takes them."""
    rng = np.random.default_rng(seed)
    n = SCENE_N
    means = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(-4, 4, n)], 1).astype(np.float32)
    log_scales = np.log(rng.uniform(0.15, 0.9, (n, 3))).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    sh = rng.uniform(-1.0, 1.0, (n, 1, 3)).astype(np.float32)
    raw = rng.uniform(-2.0, 4.0, n).astype(np.float32)
    return dict(means=means, log_scales=log_scales, quats=quats.astype(np.float32), sh=sh, raw_opacity=raw)


SCENE_SIZES = ((64, 64), (17, 9))


def case_from_aux(name, w, h, n, projected, tile_bins, isect, g_from_c, num_visible, z):
    """A case dict from a forward's aux arrays (device read-back or the CPU oracle's), for median_ref64.walk."""
    return dict(name=name, w=int(w), h=int(h), n=int(n), projected=np.asarray(projected, np.float32),
                tile_bins=np.asarray(tile_bins).astype(np.int64), isect=np.asarray(isect).astype(np.int64),
                g_from_c=np.asarray(g_from_c).astype(np.int64), num_visible=int(num_visible),
                z=np.asarray(z, np.float32))
