"""CPU checks of tests/depth_form_scenes.py: from the oracle alone, every scene is in the launch form it is named for and
exercises what it is there to exercise; and the launchers still hold the thresholds and grid caps the scenes straddle, so
that a retune turns this module red instead of silently leaving a form of the depth backward untested."""
import os
import re

import pytest

from tests import depth_form_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "brush_amd", "csrc", name)) as f:
        return f.read()


def _body(text, head):
    """The text of the function whose definition starts with `head`, up to its closing brace in column 0."""
    i = text.index(head)
    return text[i:text.index("\n}", i)]


# ---------------------------------------------------------------------------- 1. the launchers, as text
def test_quadrant_thresholds_are_the_ones_the_scenes_straddle():
    body = _body(_source("rasterize_bwd.hip"), "static uint32_t backward_quadrants_per_wave(uint32_t tiles) {")
    m = re.search(r"return tiles >= (\d+)u \? 4u : \(tiles >= (\d+)u \? 2u : 1u\);", body)
    assert m, body
    assert (int(m.group(1)), int(m.group(2))) == (S.NQ4_TILES, S.NQ2_TILES)
    # the four forms the scenes name, deterministic mode first, are the launcher's
    src = _source("rasterize_bwd.hip")
    for line in ("if (rows) launch(NqC<4>{}, std::true_type{}, depth...);",
                 "else if (nq == 4) launch(NqC<4>{}, std::false_type{}, depth...);",
                 "else if (nq == 2) launch(NqC<2>{}, std::false_type{}, depth...);",
                 "else launch(NqC<1>{}, std::false_type{}, depth...);"):
        assert line in src, line


@pytest.mark.parametrize("launcher,kernel,grid,cap", [
    ("hipError_t launch_depth_means_grad(", "k_depth_means_grad", r"min\(ceil_div\(n, kThreads\), (\d+)u\)",
     S.MEANS_GRAD_CAP_WGS),
    ("hipError_t launch_sum_isect_depth(", "k_sum_isect_depth",
     r"min\(ceil_div\(chunks, kThreads / kWave\), (\d+)u\)", S.ISECT_DEPTH_CAP_WGS),
])
def test_grid_caps_are_the_ones_the_caps_scene_crosses(launcher, kernel, grid, cap):
    src = _source("project_bwd.hip")
    body = _body(src, launcher)
    assert f"hipLaunchKernelGGL({kernel}," in body
    m = re.search(grid, body)
    assert m and int(m.group(1)) == cap, body
    assert re.search(r"constexpr uint32_t kThreads = 256;", src)  # lanes per workgroup: the `one trip` figures below
    assert S.MEANS_GRAD_ONE_TRIP == cap * 256 if kernel == "k_depth_means_grad" else S.ISECT_DEPTH_ONE_TRIP == cap * 256


# ---------------------------------------------------------------------------- 2. the form scenes
@pytest.mark.parametrize("kind", S.FORM_SCENES)
def test_form_scene_is_in_its_form(kind):
    f = S.facts(kind)
    tiles, nq = S.expected_form(kind)
    _, w, h, _ = S.scene(kind)
    assert f["tiles"] == tiles == -(-w // 16) * -(-h // 16)
    assert nq == (4 if tiles >= S.NQ4_TILES else 2 if tiles >= S.NQ2_TILES else 1)
    assert f["visible"] > 0 and not f["overflow"]
    assert f["flip_risk"] <= S.MAX_FLIP_FRACTION, f
    print(kind, f)


def test_frames_sit_on_both_sides_of_both_switches():
    tiles = {k: v[2] for k, v in S.FRAMES.items()}
    assert tiles == dict(below2=S.NQ2_TILES - 1, at2=S.NQ2_TILES, below4=S.NQ4_TILES - 1, at4=S.NQ4_TILES)
    assert set(S.FORM_SCENES) == {f"{f}_{c}" for f in S.FRAMES for c in S.CLOUDS} and len(S.FORM_SCENES) == 8


@pytest.mark.parametrize("kind", S.DEEP_SCENES)
def test_deep_scene_walks_several_batches(kind):
    """Lists beyond one 64-record batch in at least 1000 tiles, and pixels that stop on saturation."""
    f = S.facts(kind)
    assert f["tiles_over_64"] >= S.DEEP_MIN_TILES_OVER_64, f
    assert f["saturated"] > 0.5, f


@pytest.mark.parametrize("kind", [k for k in S.FORM_SCENES if k.endswith("_sparse")])
def test_sparse_scene_has_short_lists(kind):
    """Every list shorter than one batch: partial stage flushes only, nothing saturated."""
    f = S.facts(kind)
    assert 0 < f["max_len"] < 64 and f["saturated"] == 0.0, f


# ---------------------------------------------------------------------------- 3. caps
def test_caps_scene_crosses_both_grid_caps():
    f = S.facts(S.CAPS)
    assert f["tiles"] == 1024 < S.NQ2_TILES
    assert f["visible"] > S.MEANS_GRAD_ONE_TRIP + 10_000, f
    assert f["intersections"] > S.ISECT_DEPTH_ONE_TRIP, f
    assert not f["overflow"] and f["intersections"] < S.CAPS_MAX_INTERSECTS


def test_caps_rows_behind_the_cap_carry_a_depth_gradient():
    """The second grid-stride trip of k_depth_means_grad proves something only if its rows have a v_z to add: a cloud
    of opaque splats is as large, but its deepest splats sit behind saturated pixels with v_z = 0."""
    t = S.caps_tail_facts()
    assert t["tail"] == S.facts(S.CAPS)["visible"] - S.MEANS_GRAD_ONE_TRIP
    assert t["strong"] >= 10_000, t
    print(t)
