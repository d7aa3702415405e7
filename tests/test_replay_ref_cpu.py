"""The shared reference walk (tests/replay_ref.py) against a scalar restatement of its own: one pixel at a time in plain
Python floats, written here independently of the vectorised walk (in the style of distortion_ref64.brute_force).  Five
kernels' references stand on that walk, so it is pinned directly: per pixel the same entries hit and stop, every hit's
fac = alpha T agrees to a relative 1e-12 (a scalar and a vectorised exp may differ in the last float64 bit, and a
product chain of a few hundred factors keeps that below 1e-13; the kernels' allowance unit is 2^-24, five orders above),
the float32 walk counts what contrib_ref64.emulate32 counts, and the `clamp` switch does what it says."""
import math

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import contrib_ref64
from tests import replay_ref as R

FAC_RTOL = 1e-12


@pytest.fixture(scope="module")
def cases():
    cs = CC.all_cases()
    assert len(cs) == 14
    return {c["name"]: c for c in cs}


def scalar_events(case):
    """{(y, x): [(i, "hit" or "stop", fac)]}: every entry the pixel adds or stops at, front to back."""
    w, h = int(case["w"]), int(case["h"])
    rows = [[float(v) for v in row] for row in np.asarray(case["projected"], np.float32)]
    bins, isect = case["tile_bins"], case["isect"]
    events = {}
    for y in range(h):
        for x in range(w):
            first, end = int(bins[y // 16][x // 16][0]), int(bins[y // 16][x // 16][1])
            T, mine = 1.0, []
            for i in range(first, end):
                row = rows[int(isect[i])]
                dx, dy = row[0] - (x + 0.5), row[1] - (y + 0.5)
                sigma = 0.5 * (row[2] * dx * dx + row[4] * dy * dy) + row[3] * dx * dy
                raw = row[8] * math.exp(-sigma)
                if sigma < 0.0 or raw < R.INV255:
                    continue
                alpha = min(R.CLAMP, raw)
                if T * (1.0 - alpha) <= R.T_STOP:
                    mine.append((i, "stop", 0.0))
                    break
                mine.append((i, "hit", alpha * T))
                T *= 1.0 - alpha
            events[(y, x)] = mine
    return events


def walk_events(case, clamp=True):
    """The same from replay_ref.walk64, and the final 1 - T image."""
    w, h = int(case["w"]), int(case["h"])
    proj, bins, isect, _ = R.arrays(case)
    events = {(y, x): [] for y in range(h) for x in range(w)}
    alpha_img = np.zeros((h, w))
    for tile in R.tiles(bins, h, w):
        for e in R.walk64(proj, isect, tile, clamp=clamp):
            fac = e.alpha * e.T
            for kind, mask in (("hit", e.hit), ("stop", e.stop)):
                for py, px in zip(*np.nonzero(mask)):
                    events[(int(tile.ys[py, px]), int(tile.xs[py, px]))].append(
                        (e.i, kind, float(fac[py, px]) if kind == "hit" else 0.0))
        alpha_img[tile.ys, tile.xs] = 1.0 - tile.T
    return events, alpha_img


def test_walk64_matches_the_scalar_restatement(cases):
    for name, case in cases.items():
        # float64 scalar and vector evaluation cannot decide differently: no test of the case is near its threshold
        d = contrib_ref64.decisions(case)
        assert d.size == 0 or float(d.min()) > 8.0, (name, float(d.min()))
        want, (got, _) = scalar_events(case), walk_events(case)
        assert want.keys() == got.keys(), name  # every pixel of the frame, ragged edges included, once
        hits = 0
        for p, mine in want.items():
            assert [(i, k) for i, k, _ in mine] == [(i, k) for i, k, _ in got[p]], (name, p)
            for (i, k, f), (_, _, g) in zip(mine, got[p]):
                assert abs(f - g) <= FAC_RTOL * abs(f), (name, p, i, f, g)
                hits += k == "hit"
        assert hits == int(contrib_ref64.walk(case)["hits"].sum()), name
    assert sum(len(v) for v in scalar_events(cases["random_200"]).values()) > 1000  # the restatement does walk


def test_walk32_counts_what_the_contribution_emulation_counts(cases):
    for name, case in cases.items():
        n = int(case["n"])
        proj, bins, isect, g_from_c = R.arrays(case, np.float32)
        assert proj.dtype == np.float32
        hits, stops = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for tile in R.tiles(bins, int(case["h"]), int(case["w"])):
            for e in R.walk32(proj, isect, tile):
                assert e.alpha.dtype == np.float32 and e.next_T.dtype == np.float32, name
                hits[g_from_c[e.c]] += int(e.hit.sum())
                stops[g_from_c[e.c]] += int(e.stop.sum())
        emu = contrib_ref64.emulate32(case)
        assert np.array_equal(hits, emu["hits"]) and np.array_equal(stops, emu["stops"]), name


def test_clamp_switch():
    """clamp=False is felt exactly where an alpha_u exceeds 0.999: on `clamped`, not on `one_record`."""
    for case, differs in ((CC.clamped(), True), (CC.one_record(), False)):
        (ev_on, img_on), (ev_off, img_off) = walk_events(case), walk_events(case, clamp=False)
        same = ev_on == ev_off and np.array_equal(img_on, img_off)
        assert same != differs, case["name"]


def test_ratio():
    assert R.ratio([1.0, 2.0], np.array([1.0, 2.0]), np.zeros(2)) == 0.0            # 0 / 0 = 0
    assert R.ratio([1.0, 2.5], np.array([1.0, 2.0]), np.array([0.0, 1.0])) == 0.5
    assert R.ratio([1.5, 2.0], np.array([1.0, 2.0]), np.array([0.0, 1.0])) == np.inf  # a difference at zero allowance
    assert R.ratio([np.nan, 2.0], np.array([1.0, 2.0]), np.ones(2)) == np.inf
    assert R.ratio(np.zeros(0), np.zeros(0), np.zeros(0)) == 0.0
