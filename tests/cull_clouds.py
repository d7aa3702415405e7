"""Directed clouds for the projection cull and the compaction: splats placed on the decision edges of k_project_cull.

k_project_cull (project.hip) decides per splat whether it exists for the rest of the frame, in three steps: the Phase A
prefilter (near plane and a conservative screen-bounds test that must never change a decision), the exact cull
(p_view.z > 0.01, det == 0, an empty tile bbox) and the order-preserving compaction (k_compact, k_cull_scan).  The
builders here put splats where each of those can go wrong:

  off_frame      centres 1 .. 5e4 px outside the frame, 3 sigma between 0.1 and 1.5 times that distance;
  off_frame_tight needles along the direction that saturates Phase A's bound, centres on the clamp limit of t / z;
  near_plane     view depth on the f32 neighbours of 0.01;
  extreme_scale  covariances that overflow or vanish;
  compaction     everything hidden but a chosen index set aligned to wave / round / block / scan-chunk boundaries;
  quat_norm      one off_frame cloud with |q| = 0.25 and |q| = 1.1 (inside the contract) and 2 (outside it).

Every builder returns a case: dict(cloud=<the usual cloud dict, SH degree 0>, camera=dict(position, rotation_xyzw,
fov_x, fov_y, center_uv), frame=(w, h), ...), deterministic from its arguments.  `phase_a_pass` restates Phase A in
float32 numpy, operation for operation; it and `phase_a_margin` are used ONLY to place cases and to show that the
clouds have teeth (tests/test_cull_cpu.py), never as the expected result: that is the oracle's.  Plain numpy and the
oracle's det_expf; nothing here needs a GPU.
"""
import math

import numpy as np

from oracle import oracle as O

TILE_WIDTH = 16
WAVE = 64                  # common.hpp: kWave
ROUND = 256                # project.hip: kThreads, the splats of one Phase A round
CULL_BLOCK = 1024          # project.hip: kCullBlock
SELF_SCAN_BLOCKS = 2048    # project.hip: kSelfScanBlocks, above it k_cull_scan runs in chunks of 1024 blocks
NEAR = np.float32(0.01)    # project_forward.wgsl:32

_F = np.float32


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def _unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q)).tolist()


FRAMES = ((16, 16), (100, 37), (640, 480), (1920, 1080), (33, 1000))   # all but 16x16 and 640x480 are no tile multiples
CENTERS = ((0.5, 0.5), (0.1, 0.9), (1.3, -0.2))                         # the last lies outside the image
CAMERAS = {"identity": ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]),
           "rotated": ([0.3, -0.2, -5.0], _unit([0.3, -0.5, 0.2, 0.787]))}
FOV_X_DEG = (90.0, 30.0, 120.0)
FOCAL_Y_RATIO = {"eq": 1.0, "uneq": 1.3}  # focal_y / focal_x, set through fov_y


def make_camera(w, h, center_uv, camera="identity", focal="eq", fov_x_deg=90.0):
    pos, rot = CAMERAS[camera]
    fov_x = math.radians(fov_x_deg)
    fx = O.fov_to_focal(fov_x, w)
    return dict(position=list(pos), rotation_xyzw=list(rot), fov_x=fov_x,
                fov_y=O.focal_to_fov(fx * FOCAL_Y_RATIO[focal], h), center_uv=[float(center_uv[0]), float(center_uv[1])])


def uniforms(case):
    c = case["camera"]
    return O.make_uniforms(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"], case["frame"], 0)


def _view_matrix(u):
    """Row-major 4x4 world -> view in float64, from the column-major uniform words."""
    return np.asarray(u["viewmat"], np.float64).reshape(4, 4).T


def _to_world(u, p_view):
    vm = _view_matrix(u)
    pv = np.concatenate([p_view, np.ones((p_view.shape[0], 1))], axis=1)
    return (np.linalg.inv(vm) @ pv.T).T[:, :3]


def _rand_unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _case(cloud, camera, w, h, **extra):
    return dict(cloud={k: _f32(v) for k, v in cloud.items()}, camera=camera, frame=(int(w), int(h)), **extra)


def _colours(rng, n, opac=(-3.0, 3.0)):
    return dict(sh=rng.uniform(-1.0, 1.0, (n, 1, 3)), raw_opac=rng.uniform(opac[0], opac[1], n))


# ---- Phase A, restated (project.hip: k_project_cull; splat_math.hpp: make_view_params, to_view) -----------------------

def cull_k(u):
    """make_view_params' conservative cull constant: doubles on the f32 uniform words, rounded to f32 once."""
    vm = np.asarray(u["viewmat"], np.float32).astype(np.float64)
    wf2 = 0.0
    for c in range(3):
        for r in range(3):
            wf2 += vm[c * 4 + r] * vm[c * 4 + r]
    k = 0.0
    for i in range(2):
        f, img, pc = float(_F(u["focal"][i])), float(int(u["img_size"][i])), float(_F(u["pixel_center"][i]))
        tan_fov = 0.5 * img / f
        lp, ln = (img - pc) / f + 0.3 * tan_fov, pc / f + 0.3 * tan_fov
        l = lp if lp > ln else ln
        k += f * f * (1.0 + l * l)
    return _F(k * wf2 * 1.01)


def _det_expf(x):
    return np.array([O.det_expf(float(v)) for v in np.asarray(x, np.float32)], np.float32)


def exp_max_log_scale(log_scales):
    """det_expf(max of the three log-scales) per splat, f32: the one transcendental of Phase A (callers that evaluate
    Phase A many times on one cloud pass it back in)."""
    ls = np.asarray(log_scales, np.float32)
    return _det_expf(np.maximum(ls[:, 0], np.maximum(ls[:, 1], ls[:, 2])))


def _phase_a(u, means, log_scales, k_scale=1.0, exp_smax=None):
    """(maybe after the near-plane test, maybe after the screen-bounds test, margin): f32, the kernel's operations in
    the kernel's order (no contraction)."""
    vm = np.asarray(u["viewmat"], np.float32)
    m = np.asarray(means, np.float32)
    focal, pc = np.asarray(u["focal"], np.float32), np.asarray(u["pixel_center"], np.float32)
    with np.errstate(all="ignore"):
        p = [(vm[0 * 4 + r] * m[:, 0] + vm[1 * 4 + r] * m[:, 1] + vm[2 * 4 + r] * m[:, 2]) + vm[12 + r] for r in range(3)]
        front = p[2] > NEAR
        smax = (exp_max_log_scale(log_scales) if exp_smax is None else exp_smax) * _F(1.001)
        rz = _F(1.0) / p[2]
        ck = _F(np.float64(cull_k(u)) * k_scale)
        lam = smax * smax * ck * rz * rz + _F(1.0)
        rb = _F(3.0) * np.sqrt(lam) + _F(2.0)
        cx = p[0] * rz * focal[0] + pc[0]
        cy = p[1] * rz * focal[1] + pc[1]
        wpx, hpx = _F(int(u["tile_bounds"][0]) * TILE_WIDTH), _F(int(u["tile_bounds"][1]) * TILE_WIDTH)
        rej = (cx + rb < _F(-1.0)) | (cx - rb > wpx + _F(1.0)) | (cy + rb < _F(-1.0)) | (cy - rb > hpx + _F(1.0))
        out = np.maximum(np.maximum(_F(-1.0) - cx, cx - (wpx + _F(1.0))), np.maximum(_F(-1.0) - cy, cy - (hpx + _F(1.0))))
        margin = np.maximum(out, _F(0.0)).astype(np.float64) / rb.astype(np.float64)
    return front, front & ~rej, margin


def phase_a_pass(u, means, log_scales, k_scale=1.0, exp_smax=None):
    """Bool [n]: the splat survives Phase A (it is queued for the exact cull).  k_scale scales cull_k: below 1 the
    bound is no longer conservative, which is what the teeth test uses."""
    return _phase_a(u, means, log_scales, k_scale, exp_smax)[1]


def phase_a_margin(u, means, log_scales):
    """Float64 [n]: how far the centre lies outside the frame padded by one pixel, divided by Phase A's radius bound
    rb; 0 for a centre inside.  Phase A rejects above 1 (up to the f32 rounding of its own comparisons)."""
    return _phase_a(u, means, log_scales)[2]


def pixel_centres(u, means):
    """Float64 [n,2] projected centres and [n] view depth (for placing and classifying cases only)."""
    vm = _view_matrix(u)
    m = np.asarray(means, np.float64)
    p = m @ vm[:3, :3].T + vm[:3, 3]
    with np.errstate(all="ignore"):
        xy = p[:, :2] / p[:, 2:3] * np.asarray(u["focal"], np.float64) + np.asarray(u["pixel_center"], np.float64)
    return xy, p[:, 2]


def centre_in_frame(u, means):
    xy, z = pixel_centres(u, means)
    w, h = int(u["img_size"][0]), int(u["img_size"][1])
    return (z > 0) & (xy[:, 0] >= 0) & (xy[:, 0] < w) & (xy[:, 1] >= 0) & (xy[:, 1] < h)


def clamp_limits(u):
    """(lim_neg, lim_pos) per axis of calc_cov2d's clamp of t / z (helpers.wgsl:127-134), float64 [2,2]."""
    out = np.empty((2, 2))
    for i in range(2):
        f, img, pc = float(u["focal"][i]), float(int(u["img_size"][i])), float(u["pixel_center"][i])
        tan_fov = 0.5 * img / f
        out[i] = (pc / f + 0.3 * tan_fov, (img - pc) / f + 0.3 * tan_fov)
    return out


def clamped_share(u, means):
    """Bool [n]: t = z * clamp(x / z) of calc_cov2d is on its clamp on at least one axis."""
    vm = _view_matrix(u)
    p = np.asarray(means, np.float64) @ vm[:3, :3].T + vm[:3, 3]
    lim = clamp_limits(u)
    with np.errstate(all="ignore"):
        r = p[:, :2] / p[:, 2:3]
    return (r[:, 0] < -lim[0, 0]) | (r[:, 0] > lim[0, 1]) | (r[:, 1] < -lim[1, 0]) | (r[:, 1] > lim[1, 1])


# ---- off_frame --------------------------------------------------------------------------------------------------------

def off_frame(seed, w, h, center_uv=(0.5, 0.5), camera="identity", focal="eq", fov_x_deg=90.0, n=4000,
              min_px=1.0, max_px=5.0e4, extent=(0.1, 1.5), depth=(0.0101, 50.0), quat_scale=1.0, opac=(-3.0, 3.0),
              max_sigma_px=None, phase_a_share=0.25):
    """Centres d = min_px .. max_px pixels (log-uniform) outside the frame on a random side, 3 sigma = d * U(*extent), the
    three scales at random ratios in [1e-3, 1] (one of them 1) under a random rotation, view depth log-uniform in
    `depth`.  Built in view space and mapped to world through the inverse view matrix.  Phase A's radius bound rb is
    sqrt(cull_k) / focal = 3 .. 20 times the true extent, so with these sizes alone it would reject next to nothing:
    a share `phase_a_share` of the splats is sized against rb instead (rb = d * U(*extent)), which puts them on either
    side of Phase A's own decision.  quat_scale multiplies every (unit) quaternion; max_sigma_px caps the pixel sigma
    (the gradient case: no splat over a quarter of the frame)."""
    cam = make_camera(w, h, center_uv, camera, focal, fov_x_deg)
    case = _case({}, cam, w, h)
    u = uniforms(case)
    rng = np.random.default_rng(seed)
    fx, fy = float(u["focal"][0]), float(u["focal"][1])
    pcx, pcy = float(u["pixel_center"][0]), float(u["pixel_center"][1])
    z = np.exp(rng.uniform(np.log(depth[0]), np.log(depth[1]), n))
    d = np.exp(rng.uniform(np.log(min_px), np.log(max_px), n))
    side = rng.integers(0, 4, n)
    px = np.where(side == 0, -d, np.where(side == 1, w + d, rng.uniform(-d, w + d)))
    py = np.where(side == 2, -d, np.where(side == 3, h + d, rng.uniform(-d, h + d)))
    p_view = np.stack([(px - pcx) / fx * z, (py - pcy) / fy * z, z], axis=1)
    sig = d * rng.uniform(extent[0], extent[1], n) / 3.0
    if max_sigma_px is not None:
        sig = np.minimum(sig, max_sigma_px)
    rb_over_extent = math.sqrt(float(cull_k(u))) / min(fx, fy)
    sig = np.where(rng.random(n) < phase_a_share, sig / rb_over_extent, sig)
    s = sig * z / min(fx, fy)
    scales = s[:, None] * np.exp(rng.uniform(np.log(1e-3), 0.0, (n, 3)))
    scales[np.arange(n), rng.integers(0, 3, n)] = s
    quats = _rand_unit_quats(rng, n) * quat_scale
    case["cloud"] = {k: _f32(v) for k, v in dict(means=_to_world(u, p_view), log_scales=np.log(scales), quats=quats,
                                                 **_colours(rng, n, opac)).items()}
    return case


def _rotation_to(v):
    """Unit quaternions (w, x, y, z) whose rotation maps the x axis onto the unit vectors v [n,3]."""
    n = v.shape[0]
    ex = np.array([1.0, 0.0, 0.0])
    axis = np.cross(np.broadcast_to(ex, v.shape), v)
    s, c = np.linalg.norm(axis, axis=1), v @ ex
    fallback = np.broadcast_to(np.array([0.0, 0.0, 1.0]), v.shape)
    axis = np.where(s[:, None] > 1e-12, axis / np.maximum(s, 1e-300)[:, None], fallback)
    half = 0.5 * np.arctan2(s, c)
    q = np.concatenate([np.cos(half)[:, None], axis * np.sin(half)[:, None]], axis=1)
    assert q.shape == (n, 4)
    return q


def off_frame_tight(seed, w, h, center_uv=(0.5, 0.5), camera="identity", focal="eq", fov_x_deg=90.0, n=4000,
                    extent=(0.4, 1.6), depth=(0.05, 50.0), phase_a_share=0.25, aspect=(100.0, 150.0)):
    """The sub-class that presses on Phase A's bound lambda_max <= s_max^2 |J|_F^2 |W|_F^2: needles (the long axis
    U(*aspect) times the others) whose long axis is the top right singular vector of the projection Jacobian J at the
    centre, so that lambda_max = s_max^2 |J|_2^2; centres where x / z sits on the clamp limit of calc_cov2d or past it,
    1 .. 30 times as far outside the frame, on one axis (half of them: on both), where |J|_F takes the value cull_k
    assumes.  In pixels the long axis then points from the centre back toward the frame.  3 sigma along it = distance
    to the frame * U(*extent); for a share `phase_a_share` Phase A's bound rb takes that place, as in off_frame.
    The aspect decides whether the PIXELS of a case can be compared, not its cull: a needle that reaches the frame puts
    the pixels it touches 3 * aspect thin sigmas from its centre, the terms of sigma = 0.5 (a dx^2 + c dy^2) + b dx dy
    grow with the square of that and cancel, and alpha is good to 3 eps32 * sum |terms| in f32: ~0.02 relative at
    aspect 100, ~0.7 at aspect 1000 (alpha_band_at_threshold).  OFF_FRAME_TIGHT_CASES keep alpha computable;
    OFF_FRAME_TIGHT_HARD_CASES do not and are compared on the integer state alone."""
    cam = make_camera(w, h, center_uv, camera, focal, fov_x_deg)
    case = _case({}, cam, w, h)
    u = uniforms(case)
    rng = np.random.default_rng(seed)
    f = np.array([float(u["focal"][0]), float(u["focal"][1])])
    pc = np.array([float(u["pixel_center"][0]), float(u["pixel_center"][1])])
    lim = clamp_limits(u)
    size = np.array([float(w), float(h)])
    z = np.exp(rng.uniform(np.log(depth[0]), np.log(depth[1]), n))
    ratio = np.empty((n, 2))   # x / z and y / z
    past = np.zeros((n, 2), bool)
    axis = rng.integers(0, 2, n)
    both = rng.random(n) < 0.5
    for i in range(2):
        on = (axis == i) | both
        sign_pos = rng.random(n) < 0.5
        # in pixels the clamp limits lie 0.15 * size outside the frame wherever the principal point is
        out_px = 0.15 * size[i] * np.exp(rng.uniform(0.0, np.log(30.0), n))
        edge = (np.where(sign_pos, size[i] + out_px, -out_px) - pc[i]) / f[i]
        inside = (rng.uniform(0.0, size[i], n) - pc[i]) / f[i]
        ratio[:, i] = np.where(on, edge, inside)
        past[:, i] = on
    px = ratio * f + pc
    dist = np.max(np.maximum(-px, px - size), axis=1)   # pixels outside the frame, > 0 by construction
    t = np.clip(ratio, -lim[:, 0], lim[:, 1])
    # J (2x3) at the centre with the clamped t, times z; its top right singular vector
    J = np.zeros((n, 2, 3))
    J[:, 0, 0], J[:, 1, 1] = f[0], f[1]
    J[:, 0, 2], J[:, 1, 2] = -f[0] * t[:, 0], -f[1] * t[:, 1]
    _, sv, vt = np.linalg.svd(J)
    v_view = vt[:, 0, :]
    sigma_px = dist * rng.uniform(extent[0], extent[1], n) / 3.0
    rb_over_extent = math.sqrt(float(cull_k(u))) / sv[:, 0]
    sigma_px = np.where(rng.random(n) < phase_a_share, sigma_px / rb_over_extent, sigma_px)
    s_long = sigma_px * z / sv[:, 0]
    thin = 1.0 / np.exp(rng.uniform(np.log(aspect[0]), np.log(aspect[1]), (n, 2)))
    scales = np.stack([s_long, s_long * thin[:, 0], s_long * thin[:, 1]], axis=1)
    R = _view_matrix(u)[:3, :3]
    v_world = v_view @ R      # R^T v for every row
    p_view = np.stack([ratio[:, 0] * z, ratio[:, 1] * z, z], axis=1)
    case["cloud"] = {k: _f32(v) for k, v in dict(means=_to_world(u, p_view), log_scales=np.log(scales),
                                                 quats=_rotation_to(v_world), **_colours(rng, n)).items()}
    return case


def alpha_band_at_threshold(case, oa, samples=6000, seed=0):
    """For `samples` random pixels of the oracle's forward state `oa`: the relative f32 uncertainty of alpha,
    1e-5 + 3 eps32 (|t1| + |t2| + |t3|) with t the three terms of sigma (the band of the pixel check's
    _rounding_flip_explains), of every list entry whose alpha lies within a factor 2 of the 1/255 threshold.  Float64
    array; what it says is how well f32 can compute the pixels of a case at all."""
    w, h = case["frame"]
    rng = np.random.default_rng(seed)
    tbx = oa["tile_bins"].shape[1]
    bins = oa["tile_bins"].reshape(-1, 2)
    out = []
    for _ in range(samples):
        x, y = int(rng.integers(w)), int(rng.integers(h))
        r0, r1 = int(bins[(y // 16) * tbx + x // 16, 0]), int(bins[(y // 16) * tbx + x // 16, 1])
        if r1 <= r0:
            continue
        p = oa["projected_splats"][oa["compact_gid_from_isect"][r0:r1]].astype(np.float64)
        dx, dy = p[:, 0] - (x + 0.5), p[:, 1] - (y + 0.5)
        t1, t2, t3 = 0.5 * p[:, 2] * dx * dx, 0.5 * p[:, 4] * dy * dy, p[:, 3] * dx * dy
        with np.errstate(over="ignore"):
            a = p[:, 8] * np.exp(-(t1 + t2 + t3)) * 255.0
        near = (a > 0.5) & (a < 2.0)
        out.append((1e-5 + 3.0 * 2.0 ** -24 * (np.abs(t1) + np.abs(t2) + np.abs(t3)))[near])
    return np.concatenate(out) if out else np.zeros(0)


def _off_frame_cases():
    cases = {}
    for fi, (w, h) in enumerate(FRAMES):
        for ci, cuv in enumerate(CENTERS):
            for ki, cam in enumerate(CAMERAS):
                # each frame, principal point and camera meets both focal settings
                focal = "uneq" if (fi + ci + ki) % 2 else "eq"
                cases[f"{w}x{h}_c{ci}_{cam}_{focal}"] = dict(seed=100 + 10 * fi + 2 * ci + ki, w=w, h=h, center_uv=cuv,
                                                            camera=cam, focal=focal, fov_x_deg=FOV_X_DEG[fi % 3],
                                                            n=3000 if w * h > 1_000_000 else 4000)
    return cases


OFF_FRAME_CASES = _off_frame_cases()
# the tight sub-class with a pixel check: once per frame, the principal points and cameras taken in turn.  A wide field
# of view or a principal point outside the image makes J anisotropic and a needle's projected aspect several times its
# own; these go with the small frames, where the 0.3 px^2 blur over a short distance keeps alpha computable in f32.
# tests/test_cull_cpu.py holds every case to a relative uncertainty of alpha of 0.03 at the 1/255 threshold (1.2e-4
# absolute, the pixel tolerance).
OFF_FRAME_TIGHT_CASES = {
    f"{w}x{h}_c{ci}_{cam}_{focal}": dict(seed=300 + fi, w=w, h=h, center_uv=CENTERS[ci], camera=cam, focal=focal,
                                        fov_x_deg=fov, n=3000 if w * h > 1_000_000 else 4000)
    for fi, ((w, h), ci, fov, cam, focal) in enumerate(zip(FRAMES, (0, 2, 1, 0, 1), (30.0, 120.0, 30.0, 30.0, 120.0),
                                                      ("rotated", "identity", "rotated", "identity", "rotated"),
                                                      ("eq", "uneq", "uneq", "eq", "uneq")))}

# the same sub-class where alpha is NOT computable in f32: aspects up to 1000, 90 and 120 degrees on the large frames,
# the principal point outside the image.  The cull's decisions do not depend on the aspect (lambda_max =
# s_long^2 |J|_2^2 either way), so these are compared on the integer state and the list properties, without pixels:
# two admissible f32 evaluations colour ~100 of their pixels differently (uncertainty of alpha 0.1 .. 0.9).
OFF_FRAME_TIGHT_HARD_CASES = {
    f"{w}x{h}_c{ci}_{cam}_{focal}": dict(seed=400 + fi, w=w, h=h, center_uv=CENTERS[ci], camera=cam, focal=focal,
                                        fov_x_deg=fov, n=3000 if w * h > 1_000_000 else 4000, aspect=(100.0, 1000.0))
    for fi, (w, h, ci, fov, cam, focal) in enumerate(((640, 480, 2, 90.0, "rotated", "uneq"),
                                                      (640, 480, 1, 90.0, "rotated", "uneq"),
                                                      (1920, 1080, 0, 120.0, "identity", "eq")))}

QUAT_NORM_BASE = dict(seed=99, w=640, h=480, center_uv=(0.5, 0.5), camera="identity", focal="eq", fov_x_deg=90.0, n=4000)
QUAT_NORMS_IN_CONTRACT = (0.25, 1.1)
QUAT_NORM_OUT_OF_CONTRACT = 2.0


def quat_norm(scale):
    """The QUAT_NORM_BASE off_frame cloud with every quaternion multiplied by `scale`."""
    return off_frame(quat_scale=float(scale), **QUAT_NORM_BASE)


# the gradient leg of tests/test_gpu_cull.py: 2000 splats at 200x120 on the rotated off-centre camera.  t / z reaches its
# clamp 0.15 * 200 = 30 px outside the frame on x and 0.15 * 120 = 18 px on y, so the centres sit 24 .. 45 px outside; the
# pixel sigma is capped at 13 (3 sigma = 39 px: a disc of a fifth of the frame)
GRAD_CASE = dict(seed=7, w=200, h=120, center_uv=(0.1, 0.9), camera="rotated", focal="uneq", fov_x_deg=90.0, n=2000,
                 min_px=24.0, max_px=45.0, extent=(0.5, 1.5), depth=(0.5, 50.0), opac=(-2.0, 3.0), max_sigma_px=13.0,
                 phase_a_share=0.0)


# ---- near_plane -------------------------------------------------------------------------------------------------------

NEAR_DEPTHS = np.array([np.nextafter(NEAR, _F(0.0)), NEAR, np.nextafter(NEAR, _F(1.0)), _F(0.0100001), _F(0.02)],
                       np.float32)
NEAR_DEPTHS_VISIBLE = (False, False, True, True, True)   # p_view.z > 0.01f


def near_plane(seed=0, w=96, h=64, n=3000):
    """Camera at the origin, identity rotation: p_view is the mean exactly.  Splat i has view depth NEAR_DEPTHS[i % 5];
    log-scales in [-10, -9] (0.2 .. 0.6 px at the nearest depth); x / z and y / z uniform over twice the frame, so that
    about a quarter of the centres lie inside it."""
    cam = make_camera(w, h, (0.5, 0.5), "identity", "eq", 90.0)
    case = _case({}, cam, w, h, depth_class=np.arange(n) % 5)
    u = uniforms(case)
    rng = np.random.default_rng(seed)
    z = NEAR_DEPTHS[case["depth_class"]]
    fx, fy = float(u["focal"][0]), float(u["focal"][1])
    means = np.zeros((n, 3), np.float32)
    means[:, 0] = (rng.uniform(-1.0, 1.0, n) * (w / fx)).astype(np.float32) * z
    means[:, 1] = (rng.uniform(-1.0, 1.0, n) * (h / fy)).astype(np.float32) * z
    means[:, 2] = z
    case["cloud"] = {k: _f32(v) for k, v in dict(means=means, log_scales=rng.uniform(-10.0, -9.0, (n, 3)),
                                                 quats=_rand_unit_quats(rng, n), **_colours(rng, n, (0.0, 4.0))).items()}
    return case


# ---- extreme_scale ----------------------------------------------------------------------------------------------------

EXTREME_CLASSES = ("huge", "tiny", "needle")


def extreme_scale(kind, seed=0, w=96, h=64, n=1500, huge=(20.0, 44.0), tiny=(-104.0, -80.0)):
    """Identity camera, view depth in [0.5, 30], centres over twice the frame.  huge: all three log-scales in `huge`
    (scale^2 up to 1.6e38, the covariance overflows); tiny: all three in `tiny` (the covariance vanishes, only the blur
    is left); needle: one axis in `huge`, the others at -90."""
    cam = make_camera(w, h, (0.5, 0.5), "identity", "eq", 90.0)
    case = _case({}, cam, w, h)
    u = uniforms(case)
    rng = np.random.default_rng(seed + 17 * EXTREME_CLASSES.index(kind))
    fx, fy = float(u["focal"][0]), float(u["focal"][1])
    z = rng.uniform(0.5, 30.0, n)
    means = np.stack([rng.uniform(-1.0, 1.0, n) * (w / fx) * z, rng.uniform(-1.0, 1.0, n) * (h / fy) * z, z], axis=1)
    if kind == "huge":
        ls = rng.uniform(huge[0], huge[1], (n, 3))
    elif kind == "tiny":
        ls = rng.uniform(tiny[0], tiny[1], (n, 3))
    else:
        ls = np.full((n, 3), -90.0)
        ls[np.arange(n), rng.integers(0, 3, n)] = rng.uniform(huge[0], huge[1], n)
    case["cloud"] = {k: _f32(v) for k, v in dict(means=means, log_scales=ls, quats=_rand_unit_quats(rng, n),
                                                 **_colours(rng, n)).items()}
    return case


# ---- compaction -------------------------------------------------------------------------------------------------------

COMPACTION_PATTERNS = ("first", "last", "none", "all", "wave_edges", "round_edges", "block_edges", "one_per_block")
COMPACTION_SMALL_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
# either side of the self-scan switch (2048 cull workgroups), then two and four k_cull_scan chunks
COMPACTION_LARGE_N = (SELF_SCAN_BLOCKS * CULL_BLOCK, SELF_SCAN_BLOCKS * CULL_BLOCK + 1, 2049 * CULL_BLOCK + 1,
                      3073 * CULL_BLOCK + 1)
COMPACTION_LARGE_PATTERN = "block_edges"


def compaction_indices(pattern, n):
    """The chosen (visible) index set of a pattern, ascending int64.  The `edges` patterns take the first and the last
    splat of every wave (64) / Phase A round (256) / cull workgroup (1024), the last splat of the cloud closing the
    ragged last one."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "first":
        return i[:1]
    if pattern == "last":
        return i[n - 1:]
    if pattern == "none":
        return i[:0]
    if pattern == "all":
        return i
    if pattern in ("wave_edges", "round_edges", "block_edges"):
        m = dict(wave_edges=WAVE, round_edges=ROUND, block_edges=CULL_BLOCK)[pattern]
        return i[(i % m == 0) | (i % m == m - 1) | (i == n - 1)]
    if pattern == "one_per_block":
        b = np.arange((n + CULL_BLOCK - 1) // CULL_BLOCK, dtype=np.int64)
        return np.minimum(b * CULL_BLOCK + (b * 389 + 5) % CULL_BLOCK, n - 1)   # a different lane and round per block
    raise KeyError(pattern)


def compaction(pattern, n, seed=0, w=64, h=48):
    """Identity camera; every splat 5 behind the eye except the chosen set, which sits 5 in front of it inside the
    frame with a sigma of 1 .. 3 px.  All chosen splats share one depth key, so the depth sort (stable) leaves them as
    the compaction emitted them: global_from_compact_gid is the chosen set in ascending order only if the compaction
    preserved the order, and a splat dropped or doubled at a wave, round or block seam shows in it directly."""
    cam = make_camera(w, h, (0.5, 0.5), "identity", "eq", 90.0)
    chosen = compaction_indices(pattern, n)
    case = _case({}, cam, w, h, chosen=chosen)
    u = uniforms(case)
    rng = np.random.default_rng(seed)
    fx, fy = float(u["focal"][0]), float(u["focal"][1])
    k = chosen.size
    means = np.zeros((n, 3), np.float32)
    means[:, 2] = -5.0
    zc = np.full(k, 5.0)
    means[chosen, 0] = rng.uniform(-0.45, 0.45, k) * (w / fx) * zc
    means[chosen, 1] = rng.uniform(-0.45, 0.45, k) * (h / fy) * zc
    means[chosen, 2] = zc
    ls = np.full((n, 3), np.float32(np.log(0.2)))
    ls[chosen] = np.log(rng.uniform(1.0, 3.0, (k, 1)) * zc[:, None] / fx)
    quats = np.zeros((n, 4), np.float32)
    quats[:, 0] = 1.0
    sh = np.zeros((n, 1, 3), np.float32)
    sh[chosen] = rng.uniform(-1.0, 1.0, (k, 1, 3))
    raw = np.zeros(n, np.float32)
    raw[chosen] = rng.uniform(-2.0, 2.0, k)
    case["cloud"] = dict(means=means, log_scales=_f32(ls), quats=quats, sh=sh, raw_opac=raw)
    return case
