"""The return code of every refusal of the eight backward entries (plain, depth, distortion, pose, adam, adam_pose,
records, brush_reduce_view_records), without a device: fake non-null pointers that the host never dereferences, a
17 x 9 frame, and refused calls only (an accepted call would launch).  Every refusal happens before any HIP call."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # 16-byte aligned, never dereferenced
N, CAP, W, H = 4, 8, 17, 9
INVALID, SMALL = -1, -2


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    _lib.lib()
    return _lib


def frame(L):
    """(uniforms, aux) of a valid default-mode call: every aux pointer set but isect_unsorted_pos and bwd_accum."""
    u = L.BrushUniforms()
    u.img_size[:] = [W, H]
    u.tile_bounds[:] = [2, 1]
    aux = L.BrushAux()
    for name in ("projected_splats", "uniforms_buffer", "num_intersections", "num_visible", "final_index",
                 "cum_tiles_hit", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid",
                 "compact_from_global_gid", "overflow"):
        setattr(aux, name, FAKE)
    aux.max_intersects = CAP
    return u, aux


def adam_config(L):
    return L.BrushAdamConfig(1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1.0, 0.9, 0.999, 1e-15, 1, 0, 0.0, None)


class Entry:
    """One render-backward entry: a valid argument list and where its common arguments sit."""

    def __init__(self, L, name, head, tail, required, pose=False, adam=False):
        self.name, self.call = name, getattr(L.lib(), name)
        self.u, self.aux = frame(L)
        self.cfg = adam_config(L) if adam else None
        self.bytes = L.size_query("brush_bwd_workspace_size_flags", N, W, H, 0, CAP, 0)
        self.det_bytes = L.size_query("brush_bwd_workspace_size_flags", N, W, H, 0, CAP, L.AUX_DETERMINISTIC)
        self.pose_bytes = L.size_query("brush_pose_grad_workspace_size", N)
        U, A = C.byref(self.u), C.byref(self.aux)
        self.ok = [U, A] + ([C.byref(self.cfg)] if adam else []) + head + [FAKE + 0x100, self.bytes] + tail + [None]
        self.i_ws = 2 + (1 if adam else 0) + len(head)
        self.i_v_out = self.ok.index("v_out")
        self.ok[self.i_v_out] = FAKE
        self.required = required
        self.pose, self.adam = pose, adam
        if pose:
            self.ok[self.i_ws + 4] = self.pose_bytes

    def status(self, **changes):
        args = list(self.ok)
        for i, v in changes.items():
            args[int(i[1:])] = v
        return self.call(*args)

    def with_(self, changes):
        return self.status(**{f"a{i}": v for i, v in changes.items()})


def entries(L):
    P = FAKE
    six = [P] * 6
    geom = [P, P, P, P, N, P, "v_out"]  # means, log_scales, quats, raw_opacity, n, out_img, v_out
    adam_head = [P, P, P, P, P, P, N, P, "v_out", P, P, P, None, None, None]
    return {e.name: e for e in (
        Entry(L, "brush_render_backward", geom + six, [], (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15)),
        Entry(L, "brush_render_backward_depth", geom + [P, P] + six, [],
              (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)),
        Entry(L, "brush_render_backward_distortion", geom + [P, P, "cfg", P, P] + six, [],
              (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20)),
        Entry(L, "brush_render_backward_pose", geom + [P, P] + six, [P, P, 0],
              (0, 1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15, 16, 17, 19, 20), pose=True),
        # cfg, means, log_scales, quats_fed, rotation, raw_opacity, sh, n, out_img, v_out, v_xy, moment1, moment2,
        # next_quats_fed, grad_2d_accum, xy_grad_counts
        Entry(L, "brush_render_backward_adam", adam_head, [], (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 18),
              adam=True),
        Entry(L, "brush_render_backward_adam_pose", adam_head, [P, P, 0],
              (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 18, 20, 21), pose=True, adam=True),
        Entry(L, "brush_render_backward_records", geom + [P, 16], [], (0, 1, 2, 3, 4, 5, 7, 8, 9, 11)),
    )}


@pytest.fixture(scope="module")
def E(L):
    es = entries(L)
    d = es["brush_render_backward_distortion"]
    d.dcfg = L.BrushDistortion(L.DISTORTION_NDC, 0.2, 50.0)
    d.ok[d.ok.index("cfg")] = C.byref(d.dcfg)
    return es


NAMES = ("brush_render_backward", "brush_render_backward_depth", "brush_render_backward_distortion",
         "brush_render_backward_pose", "brush_render_backward_adam", "brush_render_backward_adam_pose",
         "brush_render_backward_records")


@pytest.mark.parametrize("name", NAMES)
def test_common_refusals(L, E, name):
    e = E[name]
    for i in e.required:  # each required pointer null in turn
        assert e.with_({i: None}) == INVALID, i
    # a workspace one byte short; together with a null v_out the invalid argument is what is reported
    assert e.with_({e.i_ws + 1: e.bytes - 1}) == SMALL
    assert e.with_({e.i_ws + 1: e.bytes - 1, e.i_v_out: None}) == INVALID
    try:
        # ACCUM_ZEROED: the forward must have zeroed THIS workspace's accumulator rows
        e.aux.flags, e.aux.bwd_accum = L.AUX_ACCUM_ZEROED, FAKE + 0x4000
        assert e.with_({}) == INVALID
        assert e.with_({e.i_ws + 1: e.bytes - 1}) == SMALL  # (the size is looked at first)
        e.aux.bwd_accum = None
        assert e.with_({}) == INVALID
        e.aux.flags = 8  # an unknown flag bit
        assert e.with_({}) == INVALID
        e.aux.flags = L.AUX_ANTIALIASED | 16
        assert e.with_({}) == INVALID
        # deterministic mode: needs isect_unsorted_pos, and a larger workspace
        e.aux.flags = L.AUX_DETERMINISTIC
        assert e.with_({}) == INVALID
        e.aux.isect_unsorted_pos = FAKE
        assert e.det_bytes > e.bytes
        want = INVALID if name == "brush_render_backward_distortion" else SMALL  # the term has no deterministic mode
        assert e.with_({}) == want
        assert e.with_({e.i_ws + 1: e.det_bytes - 1}) == want
    finally:
        e.aux.flags, e.aux.bwd_accum, e.aux.isect_unsorted_pos = 0, None, None
    try:
        e.u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
        assert e.with_({e.i_ws + 1: e.bytes - 1}) == INVALID
        e.u.tile_bounds[:] = [2, 1]
        e.u.sh_degree = 5
        assert e.with_({e.i_ws + 1: e.bytes - 1}) == INVALID
    finally:
        e.u.tile_bounds[:] = [2, 1]
        e.u.sh_degree = 0


def test_depth_pairs(E):
    for name, i in (("brush_render_backward_depth", 9), ("brush_render_backward_distortion", 9),
                    ("brush_render_backward_pose", 9)):
        e = E[name]
        assert e.with_({i: None}) == INVALID        # v_depth without compact_depth
        assert e.with_({i + 1: None}) == INVALID    # compact_depth without v_depth
        assert e.with_({i: None, e.i_ws + 1: e.bytes - 1}) == INVALID
    # the two entries that need the pair refuse both missing too (the pose entry takes none: an accepted call)
    assert E["brush_render_backward_depth"].with_({9: None, 10: None}) == INVALID
    assert E["brush_render_backward_distortion"].with_({9: None, 10: None}) == INVALID


def test_distortion_term(L, E):
    e = E["brush_render_backward_distortion"]
    assert e.with_({12: FAKE + 4}) == INVALID  # stats: 16-byte aligned
    assert e.with_({13: FAKE + 2}) == INVALID  # v_distortion: 4-byte aligned
    for bad in ((2, 0.2, 50.0), (1, 0.0, 50.0), (1, 0.2, 0.2), (1, 0.2, float("inf")), (1, float("nan"), 50.0)):
        b = L.BrushDistortion(*bad)
        assert e.with_({11: C.byref(b)}) == INVALID, bad
        assert e.with_({11: C.byref(b), e.i_ws + 1: e.bytes - 1}) == INVALID, bad


def test_pose_workspace(E):
    for name in ("brush_render_backward_pose", "brush_render_backward_adam_pose"):
        e = E[name]
        vm, pw, pb = e.i_ws + 2, e.i_ws + 3, e.i_ws + 4
        assert e.with_({pw: None}) == INVALID               # v_viewmat without a pose workspace
        assert e.with_({vm: None}) == INVALID               # and the reverse
        assert e.with_({vm: None, pw: None}) == INVALID     # the pose entries are for pose gradients
        assert e.with_({pb: e.pose_bytes - 1}) == SMALL     # a pose workspace that is too small
        assert e.with_({pb: 0}) == SMALL
        # the entry looks at the pose workspace before the shared checks
        assert e.with_({pb: e.pose_bytes - 1, e.i_v_out: None}) == SMALL
        assert e.with_({pw: None, pb: 0}) == INVALID


def test_adam_forms(L, E):
    for name in ("brush_render_backward_adam", "brush_render_backward_adam_pose"):
        e = E[name]
        try:
            e.cfg.time = 0
            assert e.with_({}) == INVALID
            assert e.with_({e.i_ws + 1: e.bytes - 1}) == INVALID
        finally:
            e.cfg.time = 1
        assert e.with_({5: FAKE + 4}) == INVALID    # quats_fed: 16-byte aligned
        assert e.with_({6: FAKE + 4}) == INVALID    # rotation
        assert e.with_({15: FAKE + 4}) == INVALID   # next_quats_fed, when given
        assert e.with_({16: FAKE}) == INVALID       # grad_2d_accum without xy_grad_counts
        assert e.with_({17: FAKE}) == INVALID       # and the reverse
        lazy = L.BrushLazySh()                      # a deferred SH block with no table
        try:
            e.cfg.lazy_sh = C.pointer(lazy)
            assert e.with_({}) == INVALID
        finally:
            e.cfg.lazy_sh = None


def test_records_entry(L, E):
    e = E["brush_render_backward_records"]
    assert e.with_({9: FAKE + 4}) == INVALID   # records: 16-byte aligned
    assert e.with_({9: FAKE + 4, e.i_ws + 1: e.bytes - 1}) == INVALID
    try:
        e.aux.flags = L.AUX_ANTIALIASED
        assert e.with_({}) == INVALID
        assert e.with_({e.i_ws + 1: e.bytes - 1}) == INVALID
    finally:
        e.aux.flags = 0


def test_reduce_view_records(L):
    call = L.lib().brush_reduce_view_records
    views, rows, P = 3, 16, FAKE
    nbytes = L.size_query("brush_view_index_size", N, views)
    # records, num_views, rows_per_view, view_rows, view_offsets, campos, means, n, sh_degree, v_means, v_scales,
    # v_quats, v_sh, v_opac, view_index, view_index_bytes, stream
    ok = [P, views, rows, P, None, P, P, N, 0, P, P, P, P, P, P, nbytes, None]

    def status(changes):
        args = list(ok)
        for i, v in changes.items():
            args[i] = v
        return call(*args)

    for i in (0, 3, 5, 6, 9, 10, 11, 12, 13, 14):
        assert status({i: None}) == INVALID, i
    assert status({0: P + 4}) == INVALID            # records: 16-byte aligned
    assert status({1: 0}) == INVALID                # no views
    assert status({8: 5}) == INVALID                # SH degree
    assert status({15: nbytes - 1}) == SMALL
    assert status({15: nbytes - 1, 9: None}) == INVALID
    assert status({15: nbytes - 1, 8: 5}) == INVALID
    assert status({1: 1 << 31, 2: 2, 15: 1 << 40}) == INVALID  # packed rows: views * rows_per_view must fit 32 bits
