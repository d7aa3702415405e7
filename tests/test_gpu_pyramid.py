"""GPU checks of the device image pyramid (brush_amd/pyramid.py, brush_amd/csrc/resize.hip): the area filter and the
nearest pick against the host references of tests/pyramid_ref.py, exactly; guard bytes, refused arguments and graph
replay at the C ABI; SceneLoader levels; coarse-to-fine training pinned bit for bit against runs on host-resized
datasets; multi-scale eval; both command lines."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pyramid_ref as P
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1  # BRUSH_ERR_INVALID_ARG
GUARD = 0xA5

# (w, h) -> (ow, oh)
SHAPES = [
    ((1, 1), (1, 1)),
    ((5, 7), (1, 1)),          # the whole image under one pixel
    ((33, 31), (17, 16)),      # three taps, odd RGB row pitch
    ((123, 82), (62, 41)),
    ((128, 128), (64, 64)),
    ((128, 128), (32, 32)),
    ((130, 100), (43, 33)),    # a non-integer ratio
    ((257, 255), (17, 16)),    # 16 to 17 taps per axis
    ((64, 48), (64, 48)),      # identity
    ((64, 64), (64, 16)),      # one axis only
    ((1030, 40), (515, 20)),   # more output columns than one workgroup holds
]


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return TL._bits(t)


def _patterns(w, h, c, seed):
    ramp = ((np.arange(h)[:, None, None] * 7 + np.arange(w)[None, :, None] * 3 + np.arange(c)[None, None, :] * 50) % 256)
    return {"random": np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8),
            "zeros": np.zeros((h, w, c), np.uint8), "full": np.full((h, w, c), 255, np.uint8),
            "ramp": ramp.astype(np.uint8)}


def _depth_map(w, h, dtype, seed):
    """A depth map with "no measurement" zeros; float32 ones also carry NaN and both infinities."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint16:
        d = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    else:
        d = (rng.random((h, w), dtype=np.float32) * 10).astype(np.float32)
        flat = d.reshape(-1)
        flat[::5] = np.nan
        flat[1::7] = np.inf
        flat[2::11] = -np.inf
        flat[3::13] = np.float32(-0.0)
    d.reshape(-1)[4::3] = 0
    return d


def _as_bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------- 1. the area filter, exactly
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_area_resize_equals_the_reference(dev, src, dst, channels):
    import torch

    from brush_amd import area_resize

    (w, h), (ow, oh) = src, dst
    for name, img in _patterns(w, h, channels, 100 * w + channels).items():
        got = area_resize(torch.from_numpy(img).to(dev), (ow, oh))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, channels) and got.is_contiguous()
        want = P.area_resize_ref(img, ow, oh)
        assert np.array_equal(_np(got), want), f"{src}->{dst} x{channels} {name}"


def test_area_resize_factor_strided_input_and_bad_arguments(dev):
    import torch

    from brush_amd import area_resize, downscaled_size, nearest_resize

    img = _patterns(123, 82, 4, 5)["random"]
    t = torch.from_numpy(img).to(dev)
    for f in (1, 2, 3, 4, 8, 16):
        ow, oh = downscaled_size(123, 82, f)
        assert np.array_equal(_np(area_resize(t, factor=f)), P.area_resize_ref(img, ow, oh)), f
    # a non-contiguous view (every other column) is made contiguous; an offset view starts at an odd byte address
    assert np.array_equal(_np(area_resize(t[:, ::2], (20, 30))), P.area_resize_ref(np.ascontiguousarray(img[:, ::2]), 20, 30))
    rgb = torch.from_numpy(np.ascontiguousarray(img[..., :3])).to(dev)
    assert np.array_equal(_np(area_resize(rgb[1:], (61, 40))), P.area_resize_ref(np.ascontiguousarray(img[1:, :, :3]), 61, 40))
    d = torch.zeros((82, 123), dtype=torch.float32, device=dev)
    for call in (lambda: area_resize(t), lambda: area_resize(t, (10, 10), factor=2), lambda: area_resize(t, (124, 82)),
                 lambda: area_resize(t, (0, 5)), lambda: area_resize(t, factor=17), lambda: area_resize(t, factor=0),
                 lambda: area_resize(t.float(), factor=2), lambda: area_resize(t[..., :2], factor=2),
                 lambda: area_resize(t[0], factor=2), lambda: nearest_resize(d), lambda: nearest_resize(d, (123, 83)),
                 lambda: nearest_resize(d.double(), factor=2), lambda: nearest_resize(t, factor=2)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("channels", [3, 4])
def test_area_resize_rows_wider_than_the_staging_buffer(dev, channels):
    """12000 source columns under one workgroup are more bytes than a workgroup stages at once (32 KiB): the rows go
    through in chunks, and a lane's taps span several of them."""
    import torch

    from brush_amd import area_resize

    img = _patterns(12000, 5, channels, 8)["random"]
    for ow, oh in ((2, 2), (1, 5), (3, 1)):
        got = area_resize(torch.from_numpy(img).to(dev), (ow, oh))
        assert np.array_equal(_np(got), P.area_resize_ref(img, ow, oh)), (ow, oh)


@pytest.mark.parametrize("factor", [2, 3])
def test_area_resize_64_bit_accumulator(dev, factor):
    """4200 x 4200: 255 w h + w h / 2 = 4.507e9 > 2^32 (at 4100^2 it is 4.295e9 - 0.0003e9 < 2^32: do not shrink)."""
    import torch

    from brush_amd import area_resize

    n = 4200
    assert 255 * n * n + n * n // 2 >= 2 ** 32 > 255 * 4100 * 4100 + 4100 * 4100 // 2
    o = n // factor
    full = torch.full((n, n, 3), 255, dtype=torch.uint8, device=dev)
    assert bool((area_resize(full, (o, o)) == 255).all())
    del full
    img = np.random.default_rng(factor).integers(0, 256, (n, n, 3), dtype=np.uint8)
    got = _np(area_resize(torch.from_numpy(img).to(dev), (o, o)))
    assert np.array_equal(got, P.area_resize_blocks(img, factor, factor))


def test_area_resize_64_bit_accumulator_at_a_non_integer_ratio(dev):
    """4200^2 -> 2000 x 1999, where no weight pattern repeats: all 255 stays all 255, and a separable image
    img[r,s,c] = a[r] b[s] (c + 1), whose sum under the filter factors into (wy a)[Y] (wx b)[X] (c + 1), is exact."""
    import torch

    from brush_amd import area_resize

    n, ow, oh = 4200, 2000, 1999
    full = torch.full((n, n, 3), 255, dtype=torch.uint8, device=dev)
    assert bool((area_resize(full, (ow, oh)) == 255).all())
    del full
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 10, n), rng.integers(0, 10, n)  # a b (c + 1) <= 81 * 3 = 243
    img = (a[:, None, None] * b[None, :, None] * np.arange(1, 4)[None, None, :]).astype(np.uint8)
    S = (P.overlap_weights(n, oh) @ a)[:, None, None] * (P.overlap_weights(n, ow) @ b)[None, :, None] * np.arange(1, 4)
    want = ((S + n * n // 2) // (n * n)).astype(np.uint8)
    assert np.array_equal(_np(area_resize(torch.from_numpy(img).to(dev), (ow, oh))), want)


# ---------------------------------------------------------------------------- 2. the nearest pick
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_nearest_resize_equals_resize_nearest(dev, src, dst, dtype):
    import torch

    from brush_amd import nearest_resize
    from brush_amd.dataset import resize_nearest

    (w, h), (ow, oh) = src, dst
    d = _depth_map(w, h, dtype, 7 * w + h)
    got = nearest_resize(torch.from_numpy(d).to(dev), (ow, oh))
    assert tuple(got.shape) == (oh, ow) and got.is_contiguous()
    want = resize_nearest(d, (oh, ow))
    assert got.dtype == (torch.uint16 if dtype == np.uint16 else torch.float32)
    assert np.array_equal(_as_bits(_np(got)), _as_bits(want))


# ---------------------------------------------------------------------------- 3. the C ABI: guards, refusals, graphs
def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("src,dst", SHAPES)
def test_no_write_outside_dst(dev, src, dst):
    import torch

    from brush_amd import _lib
    from brush_amd.dataset import resize_nearest

    (w, h), (ow, oh) = src, dst
    l, pad = _lib.lib(), 4096
    for channels in (3, 4):
        img = _patterns(w, h, channels, 3)["random"]
        n = ow * oh * channels
        buf = torch.full((pad + n + pad,), GUARD, dtype=torch.uint8, device=dev)
        t = torch.from_numpy(img).to(dev)
        assert l.brush_area_resize_u8(t.data_ptr(), w, h, channels, buf.data_ptr() + pad, ow, oh, _stream()) == 0
        host = _np(buf)
        assert (host[:pad] == GUARD).all() and (host[pad + n:] == GUARD).all()
        assert np.array_equal(host[pad:pad + n].reshape(oh, ow, channels), P.area_resize_ref(img, ow, oh))
    for dtype in (np.uint16, np.float32):
        d = _depth_map(w, h, dtype, 4)
        n = ow * oh * d.itemsize
        buf = torch.full((pad + n + pad,), GUARD, dtype=torch.uint8, device=dev)
        t = torch.from_numpy(d).to(dev)
        assert l.brush_nearest_resize(t.data_ptr(), d.itemsize, w, h, buf.data_ptr() + pad, ow, oh, _stream()) == 0
        host = _np(buf)
        assert (host[:pad] == GUARD).all() and (host[pad + n:] == GUARD).all()
        assert np.array_equal(host[pad:pad + n].view(np.uint16 if dtype == np.uint16 else np.uint32).reshape(oh, ow),
                              _as_bits(resize_nearest(d, (oh, ow))))


def test_refused_arguments_write_nothing(dev):
    import torch

    from brush_amd import _lib

    l = _lib.lib()
    w, h, ow, oh = 16, 12, 8, 6
    src = torch.zeros(w * h * 4, dtype=torch.uint8, device=dev)
    dst = torch.full((w * h * 4,), GUARD, dtype=torch.uint8, device=dev)
    s, d, st = src.data_ptr(), dst.data_ptr(), _stream()
    assert l.brush_area_resize_u8(s, w, h, 3, d, ow, oh, st) == 0  # the call the refusals below vary
    dst.fill_(GUARD)
    area = [
        (None, w, h, 3, d, ow, oh), (s, w, h, 3, None, ow, oh),                      # a NULL pointer
        (s, 0, h, 3, d, ow, oh), (s, w, 0, 3, d, ow, oh), (s, w, h, 3, d, 0, oh), (s, w, h, 3, d, ow, 0),  # a zero size
        (s, w, h, 3, d, w + 1, oh), (s, w, h, 3, d, ow, h + 1),                      # growing
        (s, 16385, h, 3, d, ow, oh), (s, w, 16385, 3, d, ow, oh),                    # a side above 16384
        (s, w, h, 0, d, ow, oh), (s, w, h, 1, d, ow, oh), (s, w, h, 2, d, ow, oh), (s, w, h, 5, d, ow, oh),  # channels
        (s, w, h, 3, s, ow, oh), (s, w, h, 3, s + w * h * 3 - 1, ow, oh), (s + 10, w, h, 3, s, ow, oh),     # overlap
    ]
    for args in area:
        assert l.brush_area_resize_u8(*args, st) == INVALID_ARG, args
    nearest = [
        (None, 4, w, h, d, ow, oh), (s, 4, w, h, None, ow, oh),
        (s, 4, 0, h, d, ow, oh), (s, 4, w, 0, d, ow, oh), (s, 4, w, h, d, 0, oh), (s, 4, w, h, d, ow, 0),
        (s, 4, w, h, d, w + 1, oh), (s, 4, w, h, d, ow, h + 1),
        (s, 4, 16385, h, d, ow, oh), (s, 4, w, 16385, d, ow, oh),
        (s, 0, w, h, d, ow, oh), (s, 1, w, h, d, ow, oh), (s, 3, w, h, d, ow, oh), (s, 8, w, h, d, ow, oh),  # elem_bytes
        (s, 4, w, h, s, ow, oh), (s, 2, w, h, s + w * h * 2 - 2, ow, oh), (s + 8, 4, w, h, s, ow, oh),
    ]
    for args in nearest:
        assert l.brush_nearest_resize(*args, st) == INVALID_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((src == 0).all())
    # ranges that touch without overlapping are fine
    assert l.brush_area_resize_u8(s, w, h, 3, s + w * h * 3, ow, oh, st) == 0
    assert l.brush_nearest_resize(s, 2, w, h, s + w * h * 2, ow, oh, st) == 0
    torch.cuda.synchronize()


def test_graph_replay_gives_the_eager_bits(dev):
    import torch

    from brush_amd import area_resize, nearest_resize

    img = torch.from_numpy(_patterns(130, 100, 3, 9)["random"]).to(dev)
    dep = torch.from_numpy(_depth_map(130, 100, np.float32, 9)).to(dev)
    eager = area_resize(img, (43, 33)), nearest_resize(dep, (43, 33))
    again = area_resize(img, (43, 33)), nearest_resize(dep, (43, 33))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        area_resize(img, (43, 33)), nearest_resize(dep, (43, 33))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a, d = area_resize(img, (43, 33)), nearest_resize(dep, (43, 33))
    for _ in range(2):
        a.zero_(), d.zero_()
        g.replay()
        torch.cuda.synchronize()
        for x in (eager, again):
            assert np.array_equal(_np(a), _np(x[0])) and np.array_equal(_bits(d), _bits(x[1]))
    assert np.array_equal(_np(a), P.area_resize_ref(_np(img), 43, 33))


# ---------------------------------------------------------------------------- 4. SceneLoader levels
def _with_depth(views):
    """The views with depth maps in millimetres (depth_scale 0.001) around the cameras' distance to the cloud: uint16
    for the even views, float32 for the odd ones, both with "no measurement" zeros."""
    out = []
    for i, v in enumerate(views):
        h, w = v.image.shape[:2]
        rng = np.random.default_rng(1000 + i)
        mm = rng.integers(3200, 4800, (h, w))
        mm[rng.random((h, w)) < 0.2] = 0
        out.append(dataclasses.replace(v, depth=mm.astype(np.uint16 if i % 2 == 0 else np.float32), depth_scale=0.001))
    return out


def _resized(views, factor):
    """The same views and cameras holding the host references of their images and depth maps at 1 / factor."""
    from brush_amd.dataset import resize_nearest
    from brush_amd.pyramid import downscaled_size

    out = []
    for v in views:
        h, w = v.image.shape[:2]
        ow, oh = downscaled_size(w, h, factor)
        depth = None if v.depth is None else resize_nearest(v.depth, (oh, ow))
        out.append(dataclasses.replace(v, image=P.area_resize_ref(np.ascontiguousarray(v.image), ow, oh), depth=depth))
    return out


@pytest.fixture(scope="module")
def scene(tmp_path_factory, dev):
    """(scene directory, Dataset with depth maps on the training views, the same at 1/2 by the host references)."""
    from brush_amd.dataset import Dataset
    from brush_amd.train_loop import load_dataset

    root = TL._write_scene(str(tmp_path_factory.mktemp("pyramid_scene")), dev)
    data, _ = load_dataset(root)
    assert len(data.train.views) == 16 and data.train.views[0].image.shape == (128, 128, 3)
    full = Dataset.from_views(_with_depth(data.train.views), data.eval.views)
    half = Dataset.from_views(_resized(full.train.views, 2), data.eval.views)
    return root, full, half


def test_scene_loader_levels(dev, scene):
    from brush_amd.scene_loader import SceneLoader

    _, full, half = scene
    loader, plain = SceneLoader(full.train, 3, dev), SceneLoader(full.train, 3, dev)
    own_images, own_depths = list(loader.images), list(loader.depths)
    assert loader.downscale == 1 and loader.level_bytes == 0
    total = loader.total_bytes
    assert total == sum(v.image.nbytes + v.depth.nbytes for v in full.train.views)
    with pytest.raises(ValueError):
        loader.set_downscale(0)
    with pytest.raises(ValueError):
        loader.set_downscale(17)

    loader.set_downscale(2)
    assert loader.downscale == 2 and loader.total_bytes == total
    level = 0
    for _ in range(48):
        i, view, img = loader.next_indexed()
        j, pview, pimg = plain.next_indexed()
        assert i == j and view is pview and pimg is plain.images[j]  # the draw does not depend on the level
        want = half.train.views[i]
        assert np.array_equal(_np(img), want.image)
        assert np.array_equal(_as_bits(_np(loader.depth(i))), _as_bits(want.depth))
    for i in range(16):
        assert np.array_equal(_np(loader._images[i]), half.train.views[i].image)
        level += loader._images[i].numel() + loader.depth(i).numel() * loader.depth(i).element_size()
    assert loader.level_bytes == level == sum(v.image.nbytes + v.depth.nbytes for v in half.train.views)

    loader.set_downscale(4)  # drops the half level
    assert loader.level_bytes == sum(32 * 32 * 3 + 32 * 32 * v.depth.itemsize for v in full.train.views)
    loader.set_downscale(1)
    assert loader.downscale == 1 and loader.level_bytes == 0
    for _ in range(8):
        i, _, img = loader.next_indexed()
        j, _, _ = plain.next_indexed()
        assert i == j and img is own_images[i] and loader.depth(i) is own_depths[i]
    view, img = loader.next_batch()
    assert img is own_images[full.train.views.index(view)]


# ---------------------------------------------------------------------------- 5. training
KEYS = ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")


def _train(data, steps=24, **cfg_kw):
    from brush_amd import TrainConfig
    from brush_amd.train_loop import train_scene

    cfg = TrainConfig(warmup_steps=5, refine_every=10, **cfg_kw)
    splats, log = train_scene(data, cfg, steps=steps, init_count=1000, sh_degree=3, seed=9)
    return log, {k: _bits(getattr(splats, k)) for k in KEYS}


def _same_run(a, b):
    (log_a, state_a), (log_b, state_b) = a, b
    assert np.isfinite(log_a.losses).all() and log_a.losses.shape == log_b.losses.shape
    assert np.array_equal(log_a.losses.view(np.int32), log_b.losses.view(np.int32))
    for k in KEYS:
        assert np.array_equal(state_a[k], state_b[k]), k
    assert log_a.exposures == log_b.exposures


def test_schedule_of_factor_one_is_the_run_without_one(dev, deterministic, scene):
    _, full, _ = scene
    on, off = _train(full, downscale_schedule=((0, 1),), depth_weight=0.3), _train(full, depth_weight=0.3)
    _same_run(on, off)
    assert on[0].downscales == [] and off[0].downscales == [] and on[0].to_json()["downscales"] == []


@pytest.mark.parametrize("option", [dict(depth_weight=0.3), dict(exposure_opt=True)])
def test_constant_half_schedule_is_the_run_on_the_host_resized_dataset(dev, deterministic, scene, option):
    """Loader, loop and kernels together against the host definition: training at 1/2 from step 0 gives, bit for bit, the
    loss log and the splats of a run without a schedule on the views' reference-resized images and depth maps."""
    _, full, half = scene
    on, ref = _train(full, downscale_schedule=((0, 2),), **option), _train(half, **option)
    _same_run(on, ref)
    assert on[0].downscales == [(0, 2)] and ref[0].downscales == []
    assert on[0].to_json()["downscales"] == [[0, 2]]
    if "exposure_opt" in option:
        assert on[0].exposures is not None and len(on[0].exposures) == 16
    full_res = _train(full, **option)  # and the level matters: the full-size run is another run
    assert not np.array_equal(full_res[0].losses, on[0].losses)


def test_schedule_switches_levels_through_the_loop(dev, scene):
    import torch

    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop

    _, full, _ = scene
    cfg = TrainConfig(warmup_steps=5, refine_every=50, depth_weight=0.3, downscale_schedule=((0, 4), (6, 2), (12, 1)))
    loop = TrainLoop(full, cfg, steps=18, init_count=1000, seed=2)
    assert loop.loader.downscale == 1 and loop.log.image_bytes == loop.loader.total_bytes
    for step in range(18):
        loop.step()
        want = 4 if step < 6 else (2 if step < 12 else 1)
        assert loop.loader.downscale == want, step
        assert loop.loader.level_bytes == (0 if want == 1 else sum(
            (128 // want) ** 2 * (3 + v.depth.itemsize) for v in full.train.views))
        if step == 8:  # in the middle of the half level: evals stay at the eval views' full size
            row, stats = loop.evaluate()
            assert row.step == 9 and len(stats.samples) == 4
            assert all(tuple(s.rendered.shape) == (128, 128, 3) for s in stats.samples)
            assert np.isfinite(row.psnr) and loop.loader.downscale == 2
    _, log = loop.finish()
    assert log.downscales == [(0, 4), (6, 2), (12, 1)] and log.to_json()["downscales"] == [[0, 4], [6, 2], [12, 1]]
    assert log.losses.shape == (18,) and np.isfinite(log.losses).all()
    with pytest.raises(ValueError):
        TrainLoop(full, TrainConfig(downscale_schedule=((5, 2), (5, 1))), steps=4, init_count=100)
    torch.cuda.synchronize()


def test_level_switches_do_not_synchronise(dev, scene):
    import torch

    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop

    _, full, _ = scene
    cfg = TrainConfig(warmup_steps=5, refine_every=50, depth_weight=0.3, downscale_schedule=((3, 2), (6, 4), (9, 1)))
    loop = TrainLoop(full, cfg, steps=30, init_count=1000, seed=1)
    loop.step()  # the first step fills the deferred-SH table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the mode sees a readback on this torch build
            loop.losses[0].item()
        for _ in range(12):  # steps 1..12: the switches at 3, 6 and 9, before the first refinement
            loop.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loop.trainer.last_refine is None and loop.done == 13
    _, log = loop.finish()
    assert log.downscales == [(3, 2), (6, 4), (9, 1)] and np.isfinite(log.losses[:13]).all()


# ---------------------------------------------------------------------------- 6. eval
def test_eval_at_half_size_is_eval_on_the_host_resized_scene(dev, deterministic, scene):
    from brush_amd import Splats
    from brush_amd.dataset import Scene
    from brush_amd.eval import eval_stats

    _, full, _ = scene
    views = full.eval.views + full.train.views[:2]
    splats = Splats.from_random_config(2000, 3, (np.full(3, -0.8), np.full(3, 0.8)), np.random.default_rng(4), dev)
    for f in (2, 3):
        got = eval_stats(splats, Scene(views), downscale=f)
        want = eval_stats(splats, Scene(_resized(views, f)))
        assert len(got.samples) == len(want.samples) == 6
        for a, b in zip(got.samples, want.samples):
            assert a.psnr == b.psnr and a.ssim == b.ssim and np.isfinite([a.psnr, a.ssim]).all()
            assert tuple(a.rendered.shape) == tuple(b.rendered.shape) == (b.view.image.shape[0], b.view.image.shape[1], 3)
    one, plain = eval_stats(splats, Scene(views), downscale=1), eval_stats(splats, Scene(views))
    for a, b in zip(one.samples, plain.samples):
        assert a.psnr == b.psnr and a.ssim == b.ssim and tuple(a.rendered.shape) == (128, 128, 3)
    with pytest.raises(ValueError):
        eval_stats(splats, Scene(views), downscale=0)


# ---------------------------------------------------------------------------- 7. command lines
def test_cli_schedule_and_multi_scale_eval(scene, tmp_path):
    root = scene[0]
    ply, log_json, eval_json = str(tmp_path / "out.ply"), str(tmp_path / "log.json"), str(tmp_path / "eval.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", root, "--steps", "12", "--init-count", "500",
                        "--downscale-schedule", "0:2,6:1", "--export", ply, "--json", log_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(log_json) as f:
        log = json.load(f)
    assert log["downscales"] == [[0, 2], [6, 1]] and len(log["losses"]) == 12
    r = subprocess.run([sys.executable, "-m", "brush_amd.eval", ply, root, "--downscale", "1,2", "--json", eval_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 10 and [ln.split("\t")[0] for ln in lines] == ["scale 1/1"] * 5 + ["scale 1/2"] * 5
    with open(eval_json) as f:
        res = json.load(f)
    assert [s["downscale"] for s in res["scales"]] == [1, 2]
    for s in res["scales"]:
        assert len(s["views"]) == 4 and np.isfinite([s["mean_psnr"], s["mean_ssim"]]).all()
    assert res["views"] == res["scales"][0]["views"] and res["mean_psnr"] == res["scales"][0]["mean_psnr"]
