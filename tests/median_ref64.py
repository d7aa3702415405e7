"""Float64 reference of brush_render_median_depth (brush_amd/csrc/median_depth.hip) and its gate.

The walk is the one of tests/replay_ref.py (inputs, constants and allowances; C_CONTRIB is contrib_ref64's), on a case
with a float32 z per compact id (tests/median_cases.py).  Per pixel the median entry is the first ADDED entry with

    next_T <= t_level,      t_level = float32(1) - float32(level)      (the entry point's one f32 subtraction)

and an entry that stops the pixel is never the median.  The result is a pick, so there is no error bound on it: either
the device picks the reference's entry, or the level test that decided was closer to its threshold than float32 can
tell.  For every level test a pixel makes up to and including its crossing the reference tracks the distance

    |next_T - t_level| / (next_T rel(next_T))

with rel from replay_ref's T mechanism; a pixel whose nearest test lies within UNDECIDED = 8 allowances is undecided,
and for it the reference also finds the crossing with the threshold moved down and up by 8 allowances of each entry:
the device's pick must lie between those two list positions.  A distance of exactly 0 on exactly computed values (sigma
= 0, nothing in front, 1 - alpha exact in float32) is decided: float32 computes the same tie.
"""
import numpy as np

from tests.contrib_ref64 import C_CONTRIB
from tests.replay_ref import (CLAMP, INV255, K_EXP, K_POW, K_SIG_A, K_SIG_B, K_SIG_C, K_T, T_STOP, U,  # noqa: F401
                              arrays, tiles, walk32, walk64)

UNDECIDED = 8.0
NEVER = np.iinfo(np.int64).max  # the list position of "no entry crosses"
MUTATIONS = ("lt", "last", "stop_counts", "before")


def t_level_of(level):
    return float(np.float32(1.0) - np.float32(level))


def walk(case, level, mutate=None):
    """The reference of one case at one level.  Per pixel [h,w]: id (int64 global id of the median entry, -1: none),
    depth (float32: its z, 0: none), pos (int64: its position in isect, NEVER: none), undecided (bool), pos_lo / pos_hi
    (the crossing's position with the threshold moved up / down by UNDECIDED allowances: pos_lo <= pos <= pos_hi),
    dist (float64: the nearest level test, inf where none was made).
    mutate: one of MUTATIONS, a deliberately WRONG reference (the tests check that the gate rejects each)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    w, h = int(case["w"]), int(case["h"])
    t_level = t_level_of(level)
    proj, bins, isect, g_from_c = arrays(case)
    z = np.asarray(case["z"], np.float32)
    out = dict(id=np.full((h, w), -1, np.int64), depth=np.zeros((h, w), np.float32),
               pos=np.full((h, w), NEVER, np.int64), pos_lo=np.full((h, w), NEVER, np.int64),
               pos_hi=np.full((h, w), NEVER, np.int64), dist=np.full((h, w), np.inf))
    for tile in tiles(bins, h, w):
        ys, xs = tile.ys, tile.xs
        pos = np.full(xs.shape, NEVER, np.int64)
        pos_lo, pos_hi = pos.copy(), pos.copy()
        dist = np.full(xs.shape, np.inf)
        for e in walk64(proj, isect, tile):  # the walk goes on behind the crossing, for pos_hi
            i, next_T = e.i, e.next_T
            tested = (e.passed if mutate == "stop_counts" else e.hit)
            value = e.T if mutate == "before" else next_T
            tol = C_CONTRIB * np.maximum(next_T * e.rel_next, 1e-300)
            # computed exactly in float32 too: nothing in front, exp2(-0) = 1, alpha = o, and 1 - o representable
            exact = (e.sigma == 0.0) & (e.relT == 0.0) & (e.alpha_u <= CLAMP) & \
                (next_T.astype(np.float32).astype(np.float64) == next_T)
            d = np.where(exact & (next_T == t_level), np.inf, np.abs(next_T - t_level) / tol)
            open_ = tested & (pos == NEVER)
            dist = np.where(open_, np.minimum(dist, d), dist)
            crossed = tested & ((value < t_level) if mutate == "lt" else (value <= t_level))
            if mutate == "last":
                pos = np.where(crossed, i, pos)
            else:
                pos = np.where(crossed & (pos == NEVER), i, pos)
            pos_lo = np.where(tested & (pos_lo == NEVER) & (value - UNDECIDED * tol <= t_level), i, pos_lo)
            pos_hi = np.where(tested & (pos_hi == NEVER) & (value + UNDECIDED * tol <= t_level), i, pos_hi)
        has = pos != NEVER
        cid = isect[np.where(has, pos, 0)]
        out["id"][ys, xs] = np.where(has, g_from_c[cid], -1)
        out["depth"][ys, xs] = np.where(has, z[cid], np.float32(0.0))
        out["pos"][ys, xs], out["pos_lo"][ys, xs], out["pos_hi"][ys, xs] = pos, pos_lo, pos_hi
        out["dist"][ys, xs] = dist
    out["undecided"] = out["dist"] <= UNDECIDED
    return out


def positions_of(case, ids):
    """The list position of every pixel's global id in its tile's list (NEVER for -1, -2 for an id the list lacks)."""
    w, h = int(case["w"]), int(case["h"])
    _, bins, isect, g_from_c = arrays(case)
    ids = np.asarray(ids).astype(np.int64).reshape(h, w)
    pos = np.full((h, w), -2, np.int64)
    for tile in tiles(bins, h, w):
        first = {}
        for i in range(tile.r1 - 1, tile.r0 - 1, -1):
            first[int(g_from_c[isect[i]])] = i
        first[-1] = NEVER
        pos[tile.ys, tile.xs] = np.vectorize(lambda g: first.get(int(g), -2), otypes=[np.int64])(ids[tile.ys, tile.xs])
    return pos


def gate(case, got_id, got_depth, ref):
    """Compares a result (ids [h,w] int, depth [h,w] float32) with a reference from walk().  Every pixel is checked: a
    decided one must have the reference's id and the BITS of its depth; an undecided one an id whose list position lies
    in [pos_lo, pos_hi] and the bits of that id's z (0.0 for -1).  Returns dict(ok, bad_decided, bad_undecided,
    undecided): counts of pixels."""
    w, h = int(case["w"]), int(case["h"])
    got_id = np.asarray(got_id).astype(np.int64).reshape(h, w)
    got_bits = np.ascontiguousarray(np.asarray(got_depth, np.float32).reshape(h, w)).view(np.uint32)
    und = ref["undecided"]
    ok_dec = (got_id == ref["id"]) & (got_bits == np.ascontiguousarray(ref["depth"]).view(np.uint32))
    pos = positions_of(case, got_id)
    z = np.asarray(case["z"], np.float32)
    isect = np.asarray(case["isect"]).astype(np.int64)
    listed = (pos >= 0) & (pos != NEVER)
    z_of = np.where(listed, z[isect[np.where(listed, pos, 0)]], np.float32(0.0)).astype(np.float32)
    ok_und = (pos >= 0) & (pos >= ref["pos_lo"]) & (pos <= ref["pos_hi"]) & \
        (got_bits == np.ascontiguousarray(z_of).view(np.uint32))
    bad_dec, bad_und = int((~ok_dec & ~und).sum()), int((~ok_und & und).sum())
    return dict(ok=bad_dec == 0 and bad_und == 0, bad_decided=bad_dec, bad_undecided=bad_und, undecided=int(und.sum()))


def emulate32(case, level):
    """The kernel's arithmetic restated in numpy float32 (replay_ref.walk32: fused multiply-adds in
    float64 with one rounding, exp2 through float64): a stand-in for the device in tests that run anywhere.  Returns
    (ids [h,w] int32, depth [h,w] float32)."""
    f32 = np.float32
    w, h = int(case["w"]), int(case["h"])
    t_level = f32(1.0) - f32(level)
    proj, bins, isect, g_from_c = arrays(case, f32)
    z = np.asarray(case["z"], f32)
    ids = np.full((h, w), -1, np.int32)
    depth = np.zeros((h, w), f32)
    for tile in tiles(bins, h, w):
        open_ = np.ones(tile.xs.shape, bool)  # not crossed: the kernel retires a pixel at its crossing
        tid = np.full(tile.xs.shape, -1, np.int32)
        tz = np.zeros(tile.xs.shape, f32)
        for e in walk32(proj, isect, tile):
            if not (e.live & open_).any():
                break
            cross = e.hit & open_ & (e.next_T <= t_level)
            tid = np.where(cross, np.int32(g_from_c[e.c]), tid)
            tz = np.where(cross, z[e.c], tz)
            open_ = open_ & ~cross
        ids[tile.ys, tile.xs], depth[tile.ys, tile.xs] = tid, tz
    return ids, depth
