"""Host checks of the image pyramid's definitions (no GPU): the area-filter references of tests/pyramid_ref.py against
their own properties and each other, the directed shapes of tests/resize_cases.py against the dispatch they name,
pyramid.downscaled_size, TrainConfig's downscale schedule and the two command-line spellings."""
import numpy as np
import pytest

from tests import pyramid_ref as P
from tests import resize_cases as RC


def _img(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w,h,c", [(1, 1, 3), (7, 5, 4), (64, 48, 3)])
def test_ref_identity(w, h, c):
    img = _img(w, h, c, 1)
    assert np.array_equal(P.area_resize_ref(img, w, h), img)


@pytest.mark.parametrize("value", [0, 1, 127, 128, 255])
@pytest.mark.parametrize("size", [((5, 7), (1, 1)), ((33, 31), (17, 16)), ((130, 100), (43, 33))])
def test_ref_constant_stays_constant(value, size):
    (w, h), (ow, oh) = size
    out = P.area_resize_ref(np.full((h, w, 3), value, np.uint8), ow, oh)
    assert out.shape == (oh, ow, 3) and (out == value).all()


def test_ref_halving_is_rounded_mean_of_four():
    img = _img(2, 2, 3, 2)
    a = img.astype(np.int64)
    assert np.array_equal(P.area_resize_ref(img, 1, 1)[0, 0], (a[0, 0] + a[0, 1] + a[1, 0] + a[1, 1] + 2) >> 2)
    img = _img(128, 96, 4, 3)
    a = img.astype(np.int64)
    four = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(P.area_resize_ref(img, 64, 48), four.astype(np.uint8))


@pytest.mark.parametrize("w,h,fx,fy", [(128, 128, 2, 2), (128, 128, 4, 4), (64, 64, 1, 4), (129, 84, 3, 2), (80, 48, 16, 16)])
def test_ref_two_forms_agree(w, h, fx, fy):
    img = _img(w, h, 3, 10 * fx + fy)
    assert np.array_equal(P.area_resize_ref(img, w // fx, h // fy), P.area_resize_blocks(img, fx, fy))


def test_ref_weights():
    assert P.overlap_weights(5, 1).tolist() == [[1, 1, 1, 1, 1]]
    assert P.overlap_weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    assert P.overlap_weights(4, 4).tolist() == np.diag([4] * 4).tolist()


def test_ref_one_rounding_differs_from_two_passes():
    """The definition rounds once; a horizontal pass that rounds before the vertical one is another function."""
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 1] = 1  # sum 1: one rounding gives (1 + 2) >> 2 = 0
    assert (P.area_resize_ref(img, 1, 1) == 0).all()
    rows = (img.astype(np.int64).sum(axis=1) + 1) >> 1  # rows of 1 and 0 after a rounded horizontal pass
    assert (((rows.sum(axis=0) + 1) >> 1) == 1).all()   # and 1 after a rounded vertical one


# ---------------------------------------------------------------------------- the linear-time reference
def _sweep_shapes(count=240):
    """Seeded (w, h, ow, oh, c) with sides up to 96; every sixth pins one of ow == w, oh == h, ow == 1, oh == 1."""
    rng = np.random.default_rng(2024)
    out = []
    for i in range(count):
        w, h = (int(v) for v in rng.integers(1, 97, 2))
        ow, oh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        ow = (w, ow, 1, ow, ow, ow)[i % 6]
        oh = (oh, h, oh, 1, oh, oh)[i % 6]
        out.append((w, h, ow, oh, 3 + i % 2))
    return out


def test_integral_equals_the_dense_reference_on_a_sweep():
    shapes = _sweep_shapes()
    assert len(shapes) >= 200
    for pick in (lambda s: s[2] == s[0], lambda s: s[3] == s[1], lambda s: s[2] == 1, lambda s: s[3] == 1,
                 lambda s: 1 < s[2] < s[0] and s[0] % s[2] and 1 < s[3] < s[1] and s[1] % s[3]):
        assert sum(1 for s in shapes if pick(s)) >= 30
    for i, (w, h, ow, oh, c) in enumerate(shapes):
        img = _img(w, h, c, i) if i % 3 else RC.image(w, h, c, "coin254" if i % 2 else "coin", i)
        assert np.array_equal(P.area_resize_integral(img, ow, oh), P.area_resize_ref(img, ow, oh)), (w, h, ow, oh, c)


@pytest.mark.parametrize("size", [((257, 255), (17, 16)), ((5, 7), (1, 1)), ((64, 48), (64, 48)), ((300, 200), (299, 1)),
                                  ((130, 100), (43, 33)), ((123, 82), (62, 41))])
def test_integral_equals_the_dense_reference(size):
    (w, h), (ow, oh) = size
    for pattern in RC.PATTERNS:
        img = RC.image(w, h, 4, pattern, w)
        assert np.array_equal(P.area_resize_integral(img, ow, oh), P.area_resize_ref(img, ow, oh)), pattern


@pytest.mark.parametrize("w,h,fx,fy", [(128, 128, 2, 2), (129, 84, 3, 2), (80, 48, 16, 16), (64, 64, 1, 4), (96, 85, 32, 5),
                                       (8192, 6, 2, 3), (6, 16384, 3, 2)])  # the last two: sums past 2^32 along a side
def test_integral_equals_the_block_form(w, h, fx, fy):
    for pattern in ("random", "coin", "coin254"):
        img = RC.image(w, h, 3, pattern, fx + fy)
        assert np.array_equal(P.area_resize_integral(img, w // fx, h // fy), P.area_resize_blocks(img, fx, fy))


def test_separable_form_equals_the_integral_and_the_dense_reference():
    rng = np.random.default_rng(3)
    for w, h, ow, oh in ((33, 31, 17, 16), (130, 100, 43, 33), (64, 48, 64, 1)):
        a, b = rng.integers(0, 10, h), rng.integers(0, 10, w)
        assert np.array_equal(P._cell_sums(a, 0, oh, oh, None), P.overlap_weights(h, oh) @ a)
        assert np.array_equal(P._cell_sums(a * 10 ** 7, 0, oh, oh, None), P.overlap_weights(h, oh) @ a * 10 ** 7)  # int64
        img, want = P.area_resize_separable(a, b, np.arange(1, 4), ow, oh)
        assert img.shape == (h, w, 3) and img[5, 7, 2] == a[5] * b[7] * 3
        assert np.array_equal(want, P.area_resize_ref(img, ow, oh))
        assert np.array_equal(want, P.area_resize_integral(img, ow, oh))
        full, want = P.area_resize_separable(np.full(h, 15), np.full(w, 17), np.ones(4, int), ow, oh)
        assert (full == 255).all() and full.shape == (h, w, 4) and (want == 255).all()


@pytest.mark.parametrize("mutate", P.MUTATIONS)
def test_integral_mutations_change_the_reference(mutate):
    """Negative controls: each one-token change to the linear-time reference changes its output on a fixed image, so
    the agreement above is not the agreement of two forms that ignore the token."""
    if mutate == "half_down":  # only an exact tie, S mod D == D // 2 with D even, can tell
        w, h, ow, oh = 8, 6, 4, 3
        img = RC.image(w, h, 3, "coin", 0)
        assert RC.tie_count(P.area_sums_integral(img, ow, oh), w * h) > 0
    else:
        w, h, ow, oh = 33, 31, 17, 16
        img = _img(w, h, 3, 5)
    good = P.area_resize_integral(img, ow, oh)
    assert np.array_equal(good, P.area_resize_ref(img, ow, oh))
    assert (P.area_resize_integral(img, ow, oh, mutate=mutate) != good).any(), mutate


# ---------------------------------------------------------------------------- the directed shapes
@pytest.mark.parametrize("name", list(RC.CASES) + list(RC.LARGE_CASES))
def test_every_case_sits_in_the_regime_it_names(name):
    """If this fails after a constant of resize.hip (and of resize_cases.py) was retuned, the named case no longer
    covers its side of the switch: move the case, do not edit the expectation to what the new dispatch gives."""
    for channels in ((3, 4) if name in RC.CASES else (3,)):
        w, h, ow, oh, want = RC.expected(name, channels)
        got = RC.regime(w, h, ow, oh, channels)
        assert want and {k: got.get(k) for k in want} == want, (name, channels, got)
    assert (name in RC.TIES) == (name in RC.CASES)


def test_switches_have_a_case_on_each_side():
    def r(name, channels=3):
        return RC.regime(*RC.expected(name, channels)[:4], channels)

    a, b = r("lanes_64_at_1023"), r("lanes_256_at_1024")
    assert a["workgroups"][1] == RC.FEW_WORKGROUPS - 1 and b["workgroups"][1] == RC.FEW_WORKGROUPS
    assert [r(n)["strip_rows"] for n in ("workload_1080p", "strip_2", "strip_2_ragged", "strip_3", "strip_7_ragged",
                                         "strip_8", "strip_8_capped_ragged")] == [1, 2, 2, 3, 7, 8, 8]
    for lo, hi in (("fx31_256_lanes", "fx32_256_lanes"), ("fx127_64_lanes", "fx128_64_lanes")):  # int_slot, RGBA
        assert r(lo, 4)["kernel"] == "int" and r(hi, 4)["kernel"] == "general"
        assert r(lo, 4)["slot"][0] <= RC.MAX_LDS_VECS < r(hi, 4)["slot"][0]
    assert r("block_256_square")["fx"] * r("block_256_square")["fy"] == RC.MAX_INT_BLOCK == 32 * 8 < 17 * 16
    for n in ("acc32_strips_of_8", "acc32_chunked"):  # the largest D of the 32-bit accumulator, and the next
        w, h = RC.expected(n, 3)[:2]
        assert 255 * w * h + w * h // 2 == 4294950912 < 2 ** 32 <= 255 * w * (h + 1) + w * (h + 1) // 2
        assert RC.expected(n.replace("32", "64"), 3)[:2] == (w, h + 1)
    # the shapes the suite had before all launch 64 lanes, but for the 4200^2 ones (256 lanes, 64-bit, strips of 7)
    for (w, h), (ow, oh) in (((1030, 40), (515, 20)), ((257, 255), (17, 16)), ((12000, 5), (2, 2)), ((128, 128), (64, 64))):
        assert RC.regime(w, h, ow, oh, 4)["threads"] == 64
    old = RC.regime(4200, 4200, 2000, 1999, 3)
    assert (old["threads"], old["wide"], old["strip_rows"]) == (256, True, 7)


def test_coin_images_tie_where_the_table_says():
    """The recorded tie counts of the cases of up to 2^20 source pixels (the GPU module recounts all of them), positive
    on the three shapes picked for their ties."""
    for name in ("strip_2", "lanes_64_at_1023", "chunked_64_lanes"):
        assert min(RC.TIES[name]) > 0
    for name in RC.CASES:
        for i, channels in enumerate((3, 4)):
            w, h, ow, oh, _ = RC.expected(name, channels)
            if w * h <= 1 << 20:
                img = RC.image(w, h, channels, "coin", RC.seed_of(name, channels))
                assert img.max() == 1 and np.array_equal(RC.image(w, h, channels, "coin254", RC.seed_of(name, channels)),
                                                         img + 254)
                assert RC.tie_count(P.area_sums_integral(img, ow, oh), w * h) == RC.TIES[name][i], (name, channels)


def test_patterns_are_the_pyramid_tests_patterns():
    w, h, c = 37, 29, 4
    ramp = (np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(c)[None, None, :] * 50) % 256
    assert np.array_equal(RC.image(w, h, c, "ramp", 0), ramp.astype(np.uint8))
    assert np.array_equal(RC.image(w, h, c, "random", 9), _img(w, h, c, 9))
    assert (RC.image(w, h, c, "zeros", 0) == 0).all() and (RC.image(w, h, c, "full", 0) == 255).all()


def test_block_sum_sweep_shapes():
    assert [(fx, fy) for fx, fy, _, _ in RC.SWEEP] == [(1, 1), (2, 1), (1, 3), (3, 3), (5, 3), (15, 17), (16, 16), (32, 8),
                                                       (1, 255), (127, 2)]
    for fx, fy, small, big in RC.SWEEP:
        for threads, size in ((64, small), (256, big)):
            if size is None:
                continue
            ow, oh = size
            got = RC.regime(fx * ow, fy * oh, ow, oh, 3)
            assert (got["kernel"], got["threads"], got["fx"], got["fy"]) == ("int", threads, fx, fy), (fx, fy, got)
            assert ow * oh >= 255 * fx * fy + 1 and ow * oh * fx * fy * 3 <= 51 << 20
    assert sum(1 for s in RC.SWEEP if s[3] is not None) == 7
    for fx, fy, (ow, oh) in ((2, 1, (23, 23)), (3, 3, (48, 48)), (5, 3, (62, 62))):
        n = fx * fy
        img, sums, blocks = RC.block_sum_image(fx, fy, ow, oh)
        assert (blocks[1].sum(axis=1, dtype=np.int64) == blocks[0]).all()
        assert img.shape == (fy * oh, fx * ow, 3) and img.dtype == np.uint8
        for c in range(3):
            flat = sums[..., c].reshape(-1)
            assert set(flat.tolist()) == set(range(255 * n + 1)) and (np.diff(flat) < 0).any()
        assert np.array_equal(img.reshape(oh, fy, ow, fx, 3).sum(axis=(1, 3)), sums)
        assert np.array_equal(P.area_resize_blocks(img, fx, fy), (2 * sums + n) // (2 * n))


# ---------------------------------------------------------------------------- sizes
def test_downscaled_size():
    from brush_amd.pyramid import downscaled_size

    assert downscaled_size(1, 1, 1) == (1, 1)
    assert downscaled_size(3, 3, 2) == (2, 2)
    assert downscaled_size(82, 82, 4) == (21, 21)
    assert downscaled_size(5, 5, 8) == (1, 1)
    assert downscaled_size(1920, 1080, 8) == (240, 135)
    assert downscaled_size(123, 82, 2) == (62, 41)
    assert downscaled_size(130, 100, 3) == (43, 33)
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError):
            downscaled_size(8, 8, bad)


# ---------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("schedule", [((10, 2), (5, 1)), ((5, 2), (5, 1)), ((0, 0),), ((0, 17),), ((-1, 2),), ((0, 2.5),),
                                      ((0,),)])
def test_schedule_validation_refuses(schedule):
    from brush_amd import TrainConfig

    with pytest.raises(ValueError):
        TrainConfig(downscale_schedule=schedule).check_downscale_schedule()


def test_schedule_validation_accepts():
    from brush_amd import TrainConfig

    assert TrainConfig().check_downscale_schedule() == ()
    assert TrainConfig(downscale_schedule=[[0, 16], [7, 3], [8, 1]]).check_downscale_schedule() == ((0, 16), (7, 3), (8, 1))


def test_downscale_at():
    from brush_amd import TrainConfig

    assert [TrainConfig().downscale_at(s) for s in (0, 1, 10 ** 6)] == [1, 1, 1]
    cfg = TrainConfig(downscale_schedule=((0, 4), (6, 2), (12, 1)))
    assert [cfg.downscale_at(s) for s in (0, 1, 5, 6, 7, 11, 12, 13, 1000)] == [4, 4, 4, 2, 2, 2, 1, 1, 1]
    late = TrainConfig(downscale_schedule=((3, 8),))
    assert [late.downscale_at(s) for s in (0, 2, 3, 4)] == [1, 1, 8, 8]


# ---------------------------------------------------------------------------- command line
def _schedule(argv):
    from brush_amd.train_loop import downscale_schedule_from_args, parser

    return downscale_schedule_from_args(parser().parse_args(["scene"] + argv))


def test_cli_spellings_agree():
    assert _schedule([]) == ()
    explicit = _schedule(["--downscale-schedule", "0:4,3000:2,6000:1"])
    assert explicit == ((0, 4), (3000, 2), (6000, 1))
    assert _schedule(["--num-downscales", "2", "--resolution-schedule", "3000"]) == explicit
    assert _schedule(["--num-downscales", "2"]) == explicit  # 3000 is the default period
    assert _schedule(["--num-downscales", "3", "--resolution-schedule", "250"]) == ((0, 8), (250, 4), (500, 2), (750, 1))
    assert _schedule(["--num-downscales", "0"]) == ((0, 1),)


@pytest.mark.parametrize("argv", [
    ["--downscale-schedule", "0:2", "--num-downscales", "1"],
    ["--downscale-schedule", "0:2", "--resolution-schedule", "100"],
    ["--resolution-schedule", "100"],
    ["--num-downscales", "5"],
    ["--downscale-schedule", "0:2,0:1"],
    ["--downscale-schedule", "0-2"],
    ["--downscale-schedule", "0:32"],
])
def test_cli_conflict_and_malformed_error(argv):
    with pytest.raises(ValueError):
        _schedule(argv)


def test_cli_conflict_exits(capsys):
    from brush_amd.train_loop import main

    with pytest.raises(SystemExit) as e:
        main([__file__, "--downscale-schedule", "0:2", "--num-downscales", "1"])
    assert e.value.code == 2 and "two spellings" in capsys.readouterr().err


def test_eval_cli_scales():
    from brush_amd.eval import parse_scales

    assert parse_scales("1,2,4,8") == [1, 2, 4, 8]
    for bad in ("0", "1,17", "2;4", ""):
        with pytest.raises(ValueError):
            parse_scales(bad)
