"""The tile-binning checker has teeth, and `classify` bounds what it is used for (CPU only).

tests/test_gpu_binning.py trusts two things that no GPU is needed to test: that the shared integer check and the
oracle-free properties of tests/binning_check.py reject a wrong tile list, and that binning_clouds.classify, which
places every case in its regime, never reports a walk rectangle smaller than the tiles the splat really hits.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import binning_clouds as BC
from tests import helpers as H


def _oracle_case(name):
    c = BC.CASES[name]
    cloud = BC.case_cloud(name)
    u = H.reference_test_uniforms(c["w"], c["h"], 0)
    out, oa = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"],
                               max_intersects=c["cap"])
    return cloud, u, oa, out


@pytest.fixture(scope="module")
def group16():
    return _oracle_case("group16")


def _both_reject(got, oa, what):
    with pytest.raises(AssertionError):
        BK.assert_integer_parity(got, oa)
    with pytest.raises(AssertionError):
        BK.assert_binning_properties(got)
    print(f"rejected by both: {what}")


def test_checker_accepts_the_oracle_and_rejects_wrong_lists(group16):
    """Follows test_adam_gate_rejects_wrong_references: the oracle's own aux passes; four one-entry corruptions of it
    are each rejected by the integer check AND by the properties that use no oracle."""
    _, u, oa, _ = group16
    good = BK.oracle_arrays(oa)
    V, I = BK.assert_integer_parity(good, oa)
    BK.assert_binning_properties(good)
    assert V == 100_000 and I > 3_000_000 and not good["overflow"]
    bins = oa["tile_bins"].reshape(-1, 2).astype(np.int64)
    gids = oa["compact_gid_from_isect"]
    tbx, tby = int(u["tile_bounds"][0]), int(u["tile_bounds"][1])

    # (a) two adjacent entries of one bin swapped
    t = int(np.flatnonzero(bins[:, 1] - bins[:, 0] >= 3)[7])
    i = int(bins[t, 0]) + 1
    bad = BK.oracle_arrays(oa)
    bad["compact_gid_from_isect"][[i, i + 1]] = gids[[i + 1, i]]
    _both_reject(bad, oa, "two adjacent entries of a bin swapped")

    # (b) one entry moved to the neighbouring tile: the last entry of bin t becomes the first of bin t + 1.  Chosen so
    # that it is wrong on its own terms as well: its splat's bbox does not hold tile t + 1.
    bb = BC.reference_bbox(oa["projected_splats"][:V], (tbx, tby), np.float32)
    moved = None
    for t in np.flatnonzero((bins[:-1, 1] > bins[:-1, 0]) & (bins[1:, 1] > bins[1:, 0])):
        g = int(gids[bins[t, 1] - 1])
        tx, ty = (t + 1) % tbx, (t + 1) // tbx
        if not (bb[g, 0] <= tx < bb[g, 2] and bb[g, 1] <= ty < bb[g, 3]):
            moved = int(t)
            break
    assert moved is not None
    bad = BK.oracle_arrays(oa)
    flat = bad["tile_bins"].reshape(-1, 2)
    flat[moved, 1] -= 1
    flat[moved + 1, 0] -= 1
    _both_reject(bad, oa, "one entry moved to the neighbouring tile")

    # (c) one cum_tiles_hit value off by one
    bad = BK.oracle_arrays(oa)
    bad["cum_tiles_hit"][V // 3] += 1
    _both_reject(bad, oa, "one cum_tiles_hit value off by one")

    # (d) the list truncated one entry early
    bad = BK.oracle_arrays(oa)
    bad["num_intersections"] = I - 1
    last = int(np.flatnonzero(bins[:, 1] == I)[0])
    bad["tile_bins"].reshape(-1, 2)[last, 1] = I - 1
    _both_reject(bad, oa, "the list truncated one entry early")


def test_rounding_flip_excuse_is_narrow(group16):
    """_rounding_flip_explains (the pixel check's second look, tests/test_gpu_render.py) accepts the oracle's own pixel and
    rejects the same pixel with one channel moved by 5e-4 or with another final_index, on 200 covered pixels."""
    from tests import test_gpu_render as RT

    _, u, oa, out = group16
    w, h = int(u["img_size"][0]), int(u["img_size"][1])
    rng = np.random.default_rng(3)
    n_cov = 0
    for _ in range(200):
        x, y = int(rng.integers(w)), int(rng.integers(h))
        if oa["flip_risk"][y, x] or out[y, x, 3] <= 0.05:
            continue
        n_cov += 1
        px, fin = out[y, x].astype(np.float64), int(oa["final_index"][y, x])
        assert RT._rounding_flip_explains(px, fin, x, y, oa, 1e-4)
        moved = px.copy()
        moved[n_cov % 4] += 5e-4
        assert not RT._rounding_flip_explains(moved, fin, x, y, oa, 1e-4)
        assert not RT._rounding_flip_explains(px, fin + 1, x, y, oa, 1e-4)
    assert n_cov > 100


def test_nan_equal_is_narrow(group16):
    """assert_integer_parity(nan_equal=True) lets a NaN differ in sign and payload and nothing else: a NaN moved to
    another word and a finite word changed by one ulp are both rejected; the default stays bitwise."""
    _, _, oa, _ = group16
    oa = dict(oa, projected_splats=oa["projected_splats"].copy())
    words = oa["projected_splats"].view(np.uint32)
    words[5, 2], words[9, 4] = 0x7FC00000, 0xFFC00001  # two NaNs, as `inf - inf` leaves them on the host
    good = BK.oracle_arrays(oa)
    BK.assert_integer_parity(good, oa)
    BK.assert_integer_parity(good, oa, nan_equal=True)
    flipped = BK.oracle_arrays(oa)
    flipped["projected_splats"].view(np.uint32)[5, 2] = 0xFFC00000  # the device's sign
    BK.assert_integer_parity(flipped, oa, nan_equal=True)
    with pytest.raises(AssertionError):
        BK.assert_integer_parity(flipped, oa)
    moved = BK.oracle_arrays(oa)
    w = moved["projected_splats"].view(np.uint32)
    w[5, 2], w[5, 3] = w[5, 3], w[5, 2]
    with pytest.raises(AssertionError):
        BK.assert_integer_parity(moved, oa, nan_equal=True)
    ulp = BK.oracle_arrays(oa)
    ulp["projected_splats"].view(np.uint32)[9, 3] += 1
    assert np.isfinite(ulp["projected_splats"][9, 3])
    with pytest.raises(AssertionError):
        BK.assert_integer_parity(ulp, oa, nan_equal=True)
    extra = BK.oracle_arrays(oa)
    extra["projected_splats"][11, 0] = np.nan
    with pytest.raises(AssertionError):
        BK.assert_integer_parity(extra, oa, nan_equal=True)


def test_properties_hold_on_a_truncated_list():
    """The oracle's own truncated list (flat_truncated: 1 000 003 of 2.5 M entries) passes the properties, with the
    per-splat counts bounded by, not equal to, the steps of cum_tiles_hit."""
    _, _, oa, _ = _oracle_case("flat_truncated")
    got = BK.oracle_arrays(oa)
    assert got["overflow"] == 1 and got["num_intersections"] == 1_000_003
    BK.assert_binning_properties(got)
    bad = BK.oracle_arrays(oa)
    bad["compact_gid_from_isect"][:2] = bad["compact_gid_from_isect"][[1, 0]]
    with pytest.raises(AssertionError):
        BK.assert_binning_properties(bad)


# every cloud and frame of the GPU module once (the two caps of a wide frame share both)
_CLASSIFY_CASES = [k for k in BC.CASES if k != "flat_truncated" and not k.endswith("cap9m")]


@pytest.mark.parametrize("name", _CLASSIFY_CASES)
def test_classify_never_undercounts(name):
    """classify's area is the number of tiles a walk enumerates, so it is never below the oracle's own hit count of the
    splat; its reference bbox, evaluated in f32, holds every entry of the oracle's list (the properties check that);
    and the case sits in the regime the GPU module asserts, as far as the oracle's records can tell."""
    cloud, u, oa, _ = _oracle_case(name)
    V = int(oa["num_visible"][0])
    c = BC.CASES[name]
    assert V == c["cloud"]["n"] - c["cloud"].get("n_hidden", 0)  # every splat that is not hidden is visible
    area, unknown = BC.classify(oa["projected_splats"][:V], u["tile_bounds"])
    hits = np.diff(oa["cum_tiles_hit"][:V].astype(np.int64), prepend=0)
    assert (area >= hits).all(), int((area < hits).sum())
    assert hits[area == 0].sum() == 0
    BK.assert_binning_properties(BK.oracle_arrays(oa))
    r = BC.regime(oa["projected_splats"][:V], u["tile_bounds"], cloud["means"].shape[0])
    print(name, r)
    assert r["V"] == V and r["n_small"] + r["n_mid"] + r["n_big"] == V
