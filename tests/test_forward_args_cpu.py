"""The return code of every refusal of the three forward entries (brush_render_forward, _depth, _rgba8), without a
device: fake non-null pointers that the host never dereferences, a 17 x 9 frame, and refused calls only (an accepted
call would launch).  Every refusal happens before any HIP call.  The order of the checks is pinned by two-fault calls:
an invalid argument is reported whatever the workspace's size, and a refused BrushAux::lazy_sh only behind it."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # 16-byte aligned, never dereferenced
N, CAP, W, H = 4, 8, 17, 9
INVALID, SMALL = -1, -2
AUX_POINTERS = ("projected_splats", "uniforms_buffer", "num_intersections", "num_visible", "final_index",
                "cum_tiles_hit", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid",
                "compact_from_global_gid", "overflow")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    _lib.lib()
    return _lib


class Entry:
    """One forward entry: a valid argument list (never issued as it stands) and where its arguments sit."""

    def __init__(self, L, name, outputs, own):
        self.name, self.call = name, getattr(L.lib(), name)
        self.u = L.BrushUniforms()
        self.u.img_size[:] = [W, H]
        self.u.tile_bounds[:] = [2, 1]
        self.aux = L.BrushAux()
        for p in AUX_POINTERS:  # a valid default-mode aux: every pointer set but isect_unsorted_pos, bwd_accum, lazy_sh
            setattr(self.aux, p, FAKE)
        self.aux.max_intersects = CAP
        self.bytes = L.size_query("brush_fwd_workspace_size", N, W, H, 0, CAP)
        # uniforms, means, log_scales, quats, sh_coeffs, raw_opacity, n, <outputs>, aux, workspace, bytes, stream
        self.ok = [C.byref(self.u)] + [FAKE] * 5 + [N] + outputs + [C.byref(self.aux), FAKE + 0x100, self.bytes, None]
        self.i_out = 8 if name == "brush_render_forward" else 7
        self.i_aux = 7 + len(outputs)
        self.i_ws, self.i_bytes = self.i_aux + 1, self.i_aux + 2
        self.own = own  # the entry's own outputs / pitch, checked in front of the shared checks
        self.rgba8 = name == "brush_render_forward_rgba8"

    def with_(self, changes):
        args = list(self.ok)
        for i, v in changes.items():
            args[i] = v
        return self.call(*args)

    def short(self, changes=()):
        """The call with a workspace one byte short on top of `changes`."""
        return self.with_({**dict(changes), self.i_bytes: self.bytes - 1})


NAMES = ("brush_render_forward", "brush_render_forward_depth", "brush_render_forward_rgba8")


@pytest.fixture(scope="module")
def E(L):
    pitch = int(L.lib().brush_rgba8_row_pitch(W))
    assert pitch >= W
    return {e.name: e for e in (
        Entry(L, "brush_render_forward", [0, FAKE], {}),                       # raster_u32, out_img
        Entry(L, "brush_render_forward_depth", [FAKE, FAKE, FAKE], {8: None, 9: None}),  # out_img, out_depth, compact_depth
        Entry(L, "brush_render_forward_rgba8", [FAKE, pitch], {8: W - 1}),     # out_img, row_pitch_pixels
    )}


@pytest.mark.parametrize("name", NAMES)
def test_refusals_in_order(L, E, name):
    e = E[name]
    assert e.short() == SMALL  # the one fault of the base call: what every two-fault call below is measured against
    # 1. the entry's own checks (rgba8: uniforms and pitch, depth: its two outputs), whatever the workspace's size
    for i, v in e.own.items():
        assert e.with_({i: v}) == INVALID, i
        assert e.short({i: v}) == INVALID, i
    if name == "brush_render_forward_depth":
        assert e.with_({8: None, 9: None}) == INVALID
    # 2. uniforms
    assert e.with_({0: None}) == INVALID
    assert e.short({0: None}) == INVALID
    try:
        e.u.sh_degree = 5
        assert e.with_({}) == INVALID
        assert e.short() == INVALID
        e.u.sh_degree = 0
        for bounds in ([1, 1], [2, 2], [3, 1], [0, 0]):  # not the bounds of 17 x 9
            e.u.tile_bounds[:] = bounds
            assert e.with_({}) == INVALID, bounds
            assert e.short() == INVALID, bounds
    finally:
        e.u.sh_degree = 0
        e.u.tile_bounds[:] = [2, 1]
    # aux: null, each required pointer null in turn (final_index: not required for rgba8), the flags
    assert e.with_({e.i_aux: None}) == INVALID
    assert e.short({e.i_aux: None}) == INVALID
    for p in AUX_POINTERS:
        try:
            setattr(e.aux, p, None)
            if p == "final_index" and e.rgba8:
                assert e.short() == SMALL  # accepted: the next fault is the one reported
            else:
                assert e.with_({}) == INVALID, p
                assert e.short() == INVALID, p
        finally:
            setattr(e.aux, p, FAKE)
    try:
        for flags in (8, L.AUX_ANTIALIASED | 16, 1 << 31):  # unknown flag bits
            e.aux.flags = flags
            assert e.with_({}) == INVALID, flags
            assert e.short() == INVALID, flags
        e.aux.flags = L.AUX_DETERMINISTIC  # needs isect_unsorted_pos
        assert e.with_({}) == INVALID
        assert e.short() == INVALID
        e.aux.isect_unsorted_pos = FAKE
        assert e.short() == SMALL
        e.aux.flags = L.AUX_ANTIALIASED | L.AUX_ACCUM_ZEROED  # known bits
        assert e.short() == SMALL
    finally:
        e.aux.flags, e.aux.isect_unsorted_pos = 0, None
    # out_img, workspace
    for i in (e.i_out, e.i_ws):
        assert e.with_({i: None}) == INVALID, i
        assert e.short({i: None}) == INVALID, i
    # 4. each parameter array null with n > 0 (n == 0: none is looked at)
    for i in (1, 2, 3, 4, 5):
        assert e.with_({i: None}) == INVALID, i
        assert e.short({i: None}) == INVALID, i
    bytes0 = L.size_query("brush_fwd_workspace_size", 0, W, H, 0, CAP)
    assert e.with_({1: None, 2: None, 3: None, 4: None, 5: None, 6: 0, e.i_bytes: bytes0 - 1}) == SMALL
    # 5. max_intersects == 0
    try:
        e.aux.max_intersects = 0
        assert e.with_({}) == INVALID
        assert e.with_({e.i_bytes: 0}) == INVALID
    finally:
        e.aux.max_intersects = CAP
    # 6. the workspace's size
    assert e.with_({e.i_bytes: 0}) == SMALL
    assert e.short() == SMALL


@pytest.mark.parametrize("name", NAMES)
def test_refused_lazy_sh_comes_last(L, E, name):
    """7. A BrushLazySh that make_lazy_sh refuses without reading through any pointer: no table (and, at SH degree 0,
    rows that are no whole 16-byte chunks).  Invalid with a full workspace, 'workspace too small' with a short one."""
    e = E[name]
    lazy = L.BrushLazySh()
    try:
        e.aux.lazy_sh = C.pointer(lazy)
        assert e.with_({}) == INVALID
        assert e.short() == SMALL
        e.u.sh_degree = 1  # whole chunks now: refused for the missing table alone
        bytes1 = L.size_query("brush_fwd_workspace_size", N, W, H, 1, CAP)
        assert e.with_({e.i_bytes: bytes1}) == INVALID
        assert e.with_({e.i_bytes: bytes1 - 1}) == SMALL
        lazy.table, lazy.sh_time, lazy.sh_moment1, lazy.sh_moment2 = FAKE, FAKE, FAKE, FAKE
        lazy.base, lazy.now, lazy.capacity = 5, 4, 8  # a time in front of the table
        assert e.with_({e.i_bytes: bytes1}) == INVALID
        lazy.base, lazy.now, lazy.capacity = 0, 9, 8  # and one behind it
        assert e.with_({e.i_bytes: bytes1}) == INVALID
        lazy.now, lazy.table = 8, FAKE + 4  # table: 16-byte aligned
        assert e.with_({e.i_bytes: bytes1}) == INVALID
        assert e.with_({e.i_bytes: bytes1 - 1}) == SMALL
    finally:
        e.aux.lazy_sh = None
        e.u.sh_degree = 0
