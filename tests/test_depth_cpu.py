"""CPU checks of the depth entry points: bound in the ctypes table, and argument validation before any device work."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def _uniforms(w=32, h=32):
    from brush_amd import _lib

    u = _lib.BrushUniforms()
    u.img_size[:] = [w, h]
    u.tile_bounds[:] = [-(-w // _lib.TILE_WIDTH), -(-h // _lib.TILE_WIDTH)]
    u.sh_degree = 0
    return u


def _aux():
    """Every required pointer non-null (never dereferenced: validation fails before any device work)."""
    from brush_amd import _lib

    a = _lib.BrushAux()
    for name in ("projected_splats", "uniforms_buffer", "num_intersections", "num_visible", "final_index",
                 "cum_tiles_hit", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid",
                 "compact_from_global_gid", "overflow"):
        setattr(a, name, 0x1000)
    a.max_intersects = 16
    return a


def test_depth_symbols_are_bound(lib):
    from brush_amd import _lib

    for name in ("brush_render_forward_depth", "brush_render_backward_depth"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)


def test_forward_depth_rejects_null_arguments(lib):
    from brush_amd import _lib

    u, a = _uniforms(), _aux()
    P = 0x1000  # a stand-in device address: never reached
    f = lib.brush_render_forward_depth
    assert f(None, None, None, None, None, None, 0, None, None, None, None, None, 0, None) == -1
    ok = (C.byref(u), P, P, P, P, P, 4, P, P, P, C.byref(a), P, 1 << 30, None)
    for i in (7, 8, 9, 10, 11):  # out_img, out_depth, compact_depth, aux, workspace
        args = list(ok)
        args[i] = None
        assert f(*args) == _lib.lib().brush_render_forward_depth(*args) == -1, i
    for i in (1, 2, 3, 4, 5):  # splat parameters with n > 0
        args = list(ok)
        args[i] = None
        assert f(*args) == -1, i
    bad = _uniforms()
    bad.tile_bounds[0] = 5  # not ceil(w / 16)
    assert f(C.byref(bad), *ok[1:]) == -1


def test_backward_depth_rejects_null_arguments(lib):
    u, a = _uniforms(), _aux()
    P = 0x1000
    f = lib.brush_render_backward_depth
    assert f(None, None, None, None, None, None, 0, None, None, None, None, None, None, None, None, None, None,
             None, 0, None) == -1
    ok = (C.byref(u), C.byref(a), P, P, P, P, 4, P, P, P, P, P, P, P, P, P, P, P, 1 << 30, None)
    # aux, means, log_scales, quats, raw_opacity, out_img, v_out, compact_depth, v_depth, the six gradients, workspace
    for i in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17):
        args = list(ok)
        args[i] = None
        assert f(*args) == -1, i
    det = _aux()
    det.flags = 1  # deterministic mode without isect_unsorted_pos
    assert f(ok[0], C.byref(det), *ok[2:]) == -1
