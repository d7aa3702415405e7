"""Scenes that put the depth backward (brush_render_backward_depth) into each of its launch forms and past the grid caps
of its two depth-only kernels, with the facts that make them meaningful computed from the CPU oracle alone.

The compositing backward k_rasterize_backward_quad<NQ, DET, TPB, DepthGrad> (csrc/rasterize_bwd.hip) takes NQ = 1 below
NQ2_TILES tiles, NQ = 2 from there and NQ = 4 from NQ4_TILES; deterministic mode always takes <4, DET>.  The frames
below sit on either side of both switches, each with a `sparse` cloud (lists of at most 21 entries: partial stage flushes
of one and two records) and a `deep` one (lists beyond 64 and 128 entries: several 64-record batches, the saturation
stop).  `caps` crosses the grid caps of k_depth_means_grad (MEANS_GRAD_CAP_WGS workgroups of 256 lanes, one visible
splat per lane) and k_sum_isect_depth (ISECT_DEPTH_CAP_WGS workgroups of 4 waves, 64 intersection rows per wave) in one
frame of 1024 tiles.  tests/test_depth_forms_cpu.py asserts the conditions and that the launchers still hold these
numbers; tests/test_gpu_depth_forms.py runs the scenes."""
import functools

import numpy as np

from oracle import oracle as O
from tests import helpers as H

NQ2_TILES = 1100  # backward_quadrants_per_wave: NQ = 2 from here ...
NQ4_TILES = 2304  # ... and NQ = 4 from here
MEANS_GRAD_CAP_WGS = 2048
ISECT_DEPTH_CAP_WGS = 4096
MEANS_GRAD_ONE_TRIP = MEANS_GRAD_CAP_WGS * 256        # visible splats one grid-stride trip of k_depth_means_grad covers
ISECT_DEPTH_ONE_TRIP = ISECT_DEPTH_CAP_WGS * 4 * 64   # intersection rows one trip of k_sum_isect_depth covers
CAPS_MAX_INTERSECTS = 16_000_000
EPS32 = 2.0 ** -24
C0 = np.float32(0.2820947917738781)

# kind -> (frame w, h, tiles, NQ of the default mode)
FRAMES = {
    "below2": (2512, 112, 1099, 1),
    "at2": (704, 400, 1100, 2),
    "below4": (752, 784, 2303, 2),
    "at4": (768, 768, 2304, 4),
}
CLOUDS = ("sparse", "deep")
FORM_SCENES = tuple(f"{frame}_{cloud}" for frame in FRAMES for cloud in CLOUDS)  # the eight form scenes
DEEP_SCENES = tuple(k for k in FORM_SCENES if k.endswith("_deep"))
CAPS = "caps"
MAX_FLIP_FRACTION = 1e-3
DEEP_MIN_TILES_OVER_64 = 1000


@functools.lru_cache(maxsize=None)
def _cloud(name):
    if name == "sparse":  # test_gpu_depth's `ragged` cloud
        return H.synthetic_cloud(20000, 2, seed=7, mean_mult=0.3)
    if name == "deep":
        return H.synthetic_cloud(60000, 2, seed=7, mean_mult=0.1)
    if name == CAPS:
        # 580 000 small, faint splats in a slab a few units deep, all in front of the camera: nearly all visible, no
        # pixel saturated early, so that the DEEPEST visible splats (the compact ids behind the cap) still receive a
        # depth gradient.  (Opaque splats at mean_mult 0.0005 are as many, but the deepest 15 712 sit behind saturated
        # pixels with v_z = 0: test_depth_forms_cpu.py guards against that.)
        c = H.synthetic_cloud(580000, 0, seed=7, mean_mult=0.001)
        c["log_scales"] = (c["log_scales"] - np.float32(5.0)).astype(np.float32)
        c["raw_opac"] = (c["raw_opac"] - np.float32(3.0)).astype(np.float32)
        return c
    raise ValueError(name)


def scene(kind):
    """(cloud, w, h, max_intersects) of a form scene (`<frame>_<cloud>`) or of `caps`.  The clouds are shared between
    the scenes: treat them as read-only."""
    if kind == CAPS:
        return _cloud(CAPS), 512, 512, CAPS_MAX_INTERSECTS
    frame, cloud = kind.rsplit("_", 1)
    w, h, _, _ = FRAMES[frame]
    return _cloud(cloud), w, h, None


def expected_form(kind):
    """(tiles, NQ in the default mode) the scene is built for."""
    if kind == CAPS:
        return 1024, 1
    return FRAMES[kind.rsplit("_", 1)[0]][2:]


def upstream(w, h, seed):
    """test_gpu_depth._upstream on the host: (v_out [h,w,4], v_D [h,w]) float32."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    v_out = torch.rand((h, w, 4), generator=g) - 0.5
    v_d = (torch.rand((h, w), generator=g) - 0.5) * 1e-2
    return v_out.numpy(), v_d.numpy()


def view_z(u, means):
    """Camera-space z in f32 with the projection's association (test_gpu_depth._view_z) from an oracle uniforms dict."""
    vm = np.asarray(u["viewmat"], np.float32)
    m = np.asarray(means, np.float32)
    return ((vm[2] * m[:, 0] + vm[6] * m[:, 1]) + vm[10] * m[:, 2]) + vm[14]


def twin(cloud, u):
    """The depth-as-colour twin (test_gpu_depth._twin) from an oracle uniforms dict."""
    z = view_z(u, cloud["means"])
    dc = ((z - np.float32(0.5)) / C0).astype(np.float32)
    tw = dict(cloud)
    tw["sh"] = np.repeat(dc[:, None, None], 3, axis=2).astype(np.float32)
    return tw, z


@functools.lru_cache(maxsize=None)
def oracle_forward(kind):
    """(uniforms, out_img, aux) of the scene on the CPU oracle through the reference test camera."""
    from brush_amd.render import sh_degree_from_coeffs

    cloud, w, h, cap = scene(kind)
    u = H.reference_test_uniforms(w, h, sh_degree_from_coeffs(cloud["sh"].shape[1]))
    out, aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"],
                                max_intersects=cap)
    return u, out, aux


@functools.lru_cache(maxsize=None)
def facts(kind):
    """What the oracle's forward says about a scene: tiles, visible, intersections, the tile lists' lengths, the share
    of saturated pixels (the walk stopped before its list's end) and of flip-risk pixels."""
    u, out, aux = oracle_forward(kind)
    bins = aux["tile_bins"].astype(np.int64)
    lens = (bins[..., 1] - bins[..., 0]).reshape(-1)
    w, h = int(u["img_size"][0]), int(u["img_size"][1])
    last = np.repeat(np.repeat(bins[..., 1], 16, axis=0), 16, axis=1)[:h, :w] - 1  # the last entry of the pixel's list
    nonempty = np.repeat(np.repeat(bins[..., 1] > bins[..., 0], 16, axis=0), 16, axis=1)[:h, :w]
    stopped = nonempty & (aux["final_index"].astype(np.int64) < last) & (out[..., 3] >= 0.9998)
    return dict(tiles=int(lens.size), visible=int(aux["num_visible"][0]), intersections=int(aux["num_intersections"][0]),
                overflow=bool(aux["overflow"]), max_len=int(lens.max()), tiles_over_64=int((lens > 64).sum()),
                tiles_over_128=int((lens > 128).sum()), saturated=float(stopped.mean()),
                flip_risk=float(aux["flip_risk"].astype(bool).mean()))


@functools.lru_cache(maxsize=None)
def caps_tail_facts():
    """The float64 twin backward of `caps` under v_out = 0 and the usual v_D (seed 5) on the oracle: how many of the
    compact ids behind k_depth_means_grad's first trip carry a depth gradient that the GPU test's gate resolves.
    A row is `strong` when |v_z| > 100 x 64 eps32 (|twin v_means row| + |v_z|), | | the Euclidean norm: a hundred times
    the absolute part of the allowance test_gpu_depth_forms.py grants the row (row 2 of the reference camera's W is
    (0, 0, 1))."""
    cloud, w, h, _ = scene(CAPS)
    u, _, aux = oracle_forward(CAPS)
    tw, _ = twin(cloud, u)
    t_img, t_aux = O.render_forward(u, tw["means"], tw["log_scales"], tw["quats"], tw["sh"], tw["raw_opac"],
                                    max_intersects=CAPS_MAX_INTERSECTS)
    assert int(t_aux["num_visible"][0]) == int(aux["num_visible"][0])
    vt = np.zeros((h, w, 4), np.float32)
    vt[..., 0] = upstream(w, h, 5)[1]
    g = O.render_backward_f64(u, t_aux, tw["means"], tw["log_scales"], tw["quats"], tw["raw_opac"], t_img, vt)
    V = int(aux["num_visible"][0])
    tail = aux["global_from_compact_gid"][MEANS_GRAD_ONE_TRIP:V].astype(np.int64)
    v_z = g["v_sh"][tail, 0, 0] / float(C0)
    floor = 64 * EPS32 * (np.sqrt((g["v_means"][tail] ** 2).sum(axis=1)) + np.abs(v_z))
    return dict(tail=int(tail.size), nonzero=int((v_z != 0).sum()), strong=int((np.abs(v_z) > 100.0 * floor).sum()))
