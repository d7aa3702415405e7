"""The opt-in stage profiler (brush_profiler_*, brush_amd.profiler.StageProfiler), which bench.py reads its per-stage
numbers from: an attached profiler changes no output, a stage without a launch reads exactly 0.0, stop_after ends a
pass behind a stage without recording, and a destroyed profiler is detached.  One process, a few hundred splats on a
ragged 40 x 24 frame (3 x 2 tiles), SH degree 1, default and deterministic mode.  No timing threshold anywhere."""
import ctypes as Cc
import math

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, W, HGT, DEG = 300, 40, 24, 1
NCOEF = (DEG + 1) ** 2
STAGES = ["project_cull", "depth_sort", "project_visible", "prefix_sum", "map_intersects", "tile_sort", "tile_bins",
          "rasterize", "bwd_zero", "rasterize_bwd", "project_bwd"]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True  # every buffer a pass does not write keeps its 0xCD sentinel
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene(dev):
    import torch

    import brush_amd

    cloud = H.synthetic_cloud(N, DEG, seed=4, mean_mult=0.002)  # a 20-unit cube around the origin, camera 8 in front
    p = {k: torch.as_tensor(v, device=dev) for k, v in cloud.items()}
    c = H.reference_test_camera(W, HGT)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    v_out = torch.as_tensor(np.random.default_rng(7).standard_normal((HGT, W, 4)).astype(np.float32) / (HGT * W),
                            device=dev)
    return p, cam, v_out


def forward(scene, det, **kw):
    from brush_amd import render as R

    p, cam, _ = scene
    return R._forward_impl(cam, (W, HGT), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], False, None,
                           deterministic=det, **kw)


def render(scene, det, **kw):
    """One forward and one dense backward: (image, aux, the six gradients)."""
    import torch

    from brush_amd import render as R

    p, _, v_out = scene
    out, aux, u = forward(scene, det, **kw)
    g, _ = R._backward_impl(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], NCOEF, out, v_out)
    torch.cuda.synchronize()
    return out, aux, g


def same_forward(a, b):
    import torch

    (out_a, aux_a), (out_b, aux_b) = a, b
    return (torch.equal(out_a, out_b) and torch.equal(aux_a.final_index, aux_b.final_index) and
            aux_a.read_num_visible() == aux_b.read_num_visible() and
            aux_a.read_num_intersections() == aux_b.read_num_intersections())


def check_ms(ms, zero):
    assert list(ms) == STAGES
    for name, v in ms.items():
        assert math.isfinite(v) and v >= 0.0, (name, v)
    for name in zero:
        assert ms[name] == 0.0, (name, ms[name])  # no launch, no event: exactly zero


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_attached_profiler(dev, scene, det):
    import torch

    from brush_amd.profiler import StageProfiler

    out0, aux0, g0 = render(scene, det)
    assert aux0.read_num_visible() > 0 and aux0.read_num_intersections() > 0  # every stage has work
    assert aux0.deterministic == det

    prof = StageProfiler()
    assert prof.names == STAGES
    assert list(prof.read_ms().values()) == [0.0] * 11  # nothing recorded yet
    with prof:
        out1, aux1, g1 = render(scene, det)
        # the deterministic mode has no zero-fill, and in the default mode this forward zeroed the accumulators
        ms = prof.read_ms()
        check_ms(ms, ["bwd_zero"] if det else ["tile_bins", "bwd_zero"])
        assert same_forward((out0, aux0), (out1, aux1))
        if det:  # (the default mode adds with float atomics: not compared by bits)
            for k in g0:
                assert torch.equal(g0[k], g1[k]), k
        else:  # a backward that zero-fills itself: the stage has a launch
            out2, aux2, _ = render(scene, det, expect_backward=False)
            ms = prof.read_ms()
            check_ms(ms, ["tile_bins"])
            assert same_forward((out0, aux0), (out2, aux2))

        # the pass ends behind the cull: counts written, nothing composited, nothing recorded
        prof.stop_after("project_cull")
        out3, aux3, _ = forward(scene, det)  # (_lib.check: the call returned BRUSH_OK)
        torch.cuda.synchronize()
        assert bool((out3.view(torch.uint8) == 0xCD).all())
        assert bool((aux3.final_index.view(torch.uint8) == 0xCD).all())
        assert aux3.read_num_visible() == aux0.read_num_visible()
        assert prof.read_ms() == ms  # still the previous full pass

        prof.stop_after(None)
        out4, aux4, _ = forward(scene, det)
        torch.cuda.synchronize()
        assert same_forward((out0, aux0), (out4, aux4))
    out5, aux5, _ = forward(scene, det)  # detached
    torch.cuda.synchronize()
    assert same_forward((out0, aux0), (out5, aux5))
    prof.close()


def test_stage_names_and_stop_after_range(dev, scene):
    import torch

    from brush_amd import _lib
    from brush_amd.profiler import StageProfiler

    l = _lib.lib()
    assert _lib.NUM_STAGES == 11
    assert [l.brush_stage_name(i).decode() for i in range(11)] == STAGES
    for i in (-1, 11, 12, -2, 1 << 20):
        assert l.brush_stage_name(i) == b"?"
    prof = StageProfiler()
    assert l.brush_profiler_stop_after(prof._h, _lib.NUM_STAGES) == -1  # BRUSH_ERR_INVALID_ARG
    assert l.brush_profiler_stop_after(prof._h, -2) == -1
    assert l.brush_profiler_stop_after(None, 0) == -1
    assert l.brush_profiler_stop_after(prof._h, _lib.NUM_STAGES - 1) == 0
    assert l.brush_profiler_stop_after(prof._h, -1) == 0
    assert l.brush_profiler_read(prof._h, None) == -1
    assert l.brush_profiler_read(None, (Cc.c_float * 11)()) == -1
    # the refused settings left the whole pass in place
    out0, aux0, _ = forward(scene, False)
    with prof:
        out1, aux1, _ = forward(scene, False)
    torch.cuda.synchronize()
    assert same_forward((out0, aux0), (out1, aux1))
    prof.close()


def test_destroy_detaches(dev, scene):
    import torch

    from brush_amd.profiler import StageProfiler

    out0, aux0, _ = forward(scene, False)
    prof = StageProfiler()
    prof.__enter__()  # attached ...
    prof.close()      # ... and destroyed without a detach of its own
    out1, aux1, g1 = render(scene, False)
    assert same_forward((out0, aux0), (out1, aux1))
    assert bool(torch.isfinite(g1["v_means"]).all())
