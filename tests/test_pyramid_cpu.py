"""Host checks of the image pyramid's definitions (no GPU): the area-filter reference of tests/pyramid_ref.py against
its own properties, pyramid.downscaled_size, TrainConfig's downscale schedule and the two command-line spellings."""
import numpy as np
import pytest

from tests import pyramid_ref as P


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
