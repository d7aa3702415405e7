"""Directed clouds for the tile-binning tests: splat classes chosen by the test, not by the bench distribution.

The tile-binning middle of the forward (tile_count.hip, tile_emit.hip, tile_walk.hpp and the tile sort) picks its code
paths from device-side counts: the visible count V, the number of (splat, chunk) queue items, the bbox area of every
splat.  `directed_cloud` builds a cloud whose V is known exactly and whose mix of small / mid / big / thin splats is
set by fractions, so that a case of a few hundred thousand splats sits in the regime it names.  `classify` restates
the walk rectangle in float64 and is used ONLY to assert that a case sits in that regime (it is approximate: the device
computes in f32), never for correctness.  Plain numpy; nothing here needs a GPU.
"""
import math

import numpy as np

TILE_WIDTH = 16
CHUNK_TILES = 64          # tile_walk.hpp: kChunkTiles
SMALL_AREA = 16           # kSmallArea
SMALL_AREA_MANY = 64      # kSmallAreaMany
SMALL_AREA_SWITCH = 1 << 19   # kSmallAreaSwitch: V > this -> inline walks up to 64 tiles
HALF_WAVE_SPLATS = 1 << 18    # kHalfWaveSplats: V <= this -> a wave takes 32 splats
FLAT_EMIT_MIN = 1 << 19       # kFlatEmitMin: V >= this -> wave-flattened inline emission
GROUP4_MAX = 16384            # walk_group: <= this many items -> 4 per wave
GROUP16_MAX = 1 << 18         # walk_group: <= this many items -> 16 per wave, above: 64


def directed_cloud(n, w, h, seed, fr_mid, fr_big, fr_thin, n_hidden=0, big_sigma=(19, 34), thin_aspect=50):
    """Same dict as synthetic_cloud (SH degree 0), sized for helpers.reference_test_camera: eye (0,0,-8), fov 90 deg on
    x, focal = w/2 on both axes.  Every splat that is not hidden projects inside the frame, so V = n - n_hidden.

    Classes (probabilities 1 - sum, fr_mid, fr_big, fr_thin), pixel sigma per class, scale = sigma * depth / focal:
      small  U(0.2, 4)     <= 16 bbox tiles
      mid    U(9, 17)      17-64 bbox tiles
      big    U(*big_sigma) > 64 bbox tiles, 2-3 chunks
      thin   as big, scaled by (1, 1/thin_aspect, 1/thin_aspect) and, like all, rotated about the view axis."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(4.0, 12.0, n)
    x = rng.uniform(-0.98, 0.98, n) * d
    y = rng.uniform(-0.98, 0.98, n) * d * (float(h) / float(w))
    means = np.stack([x, y, d - 8.0], axis=1)
    fr_small = 1.0 - (fr_mid + fr_big + fr_thin)
    assert fr_small > -1e-12
    p = np.array([max(fr_small, 0.0), fr_mid, fr_big, fr_thin])
    cls = rng.choice(4, size=n, p=p / p.sum())
    sigma = np.where(cls == 0, rng.uniform(0.2, 4.0, n),
                     np.where(cls == 1, rng.uniform(9.0, 17.0, n), rng.uniform(big_sigma[0], big_sigma[1], n)))
    s = sigma * d / (0.5 * float(w))
    scales = np.repeat(s[:, None], 3, axis=1)
    scales[cls == 3, 1:] /= float(thin_aspect)
    a = rng.uniform(0.0, 2.0 * math.pi, n)
    quats = np.stack([np.cos(0.5 * a), np.zeros(n), np.zeros(n), np.sin(0.5 * a)], axis=1)  # (w, x, y, z)
    raw_opac = np.where(cls == 0, rng.uniform(-6.0, 4.0, n), rng.uniform(2.0, 5.0, n))
    sh = rng.uniform(-1.0, 1.0, (n, 1, 3))
    if n_hidden:
        hidden = rng.choice(n, size=int(n_hidden), replace=False)
        means[hidden, 2] = -20.0  # 12 behind the eye
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    return dict(means=f32(means), log_scales=f32(np.log(scales)), quats=f32(quats), sh=f32(sh), raw_opac=f32(raw_opac))


# ---- the walk rectangle, restated (splat_math.hpp: radius_from_conic, get_tile_bbox, make_tile_reach, walk_rect) ------

def _trunc_clamp(x, lo, hi):
    """iclamp(f2i_sat(x), lo, hi) for finite or non-finite x (NaN -> 0)."""
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(np.trunc(np.clip(x, -2.0e9, 2.0e9)), lo, hi).astype(np.int64)


def reference_bbox(projected, tile_bounds, dtype=np.float32):
    """get_tile_bbox(xy, radius_from_conic(conic)) per record: int64 [V,4] (min.x, min.y, max.x, max.y), max
    exclusive.  With dtype=float32 every operation is the device's own (IEEE add, multiply, divide and square root in
    the same order, no contraction), so the result is the device's bbox to the bit."""
    t = dtype
    pr = np.asarray(projected)
    xy = pr[:, 0:2].astype(t)
    c0, c1, c2 = (pr[:, k].astype(t) for k in (2, 3, 4))
    with np.errstate(all="ignore"):
        det = t(1.0) / (c0 * c2 - c1 * c1)
        cx, cz = c2 * det, c0 * det
        b = t(0.5) * (cx + cz)
        sq = np.sqrt(np.maximum(t(0.1), b * b - det))
        v1, v2 = b + sq, b - sq
        radius = t(3.0) * np.sqrt(np.maximum(t(0.0), np.maximum(v1, v2)))
        radius = np.ceil(radius)
        radius = np.where(radius > 0, np.minimum(radius, t(4294967295.0)), t(0.0)).astype(t)  # f2u_sat, then (float)
        tr = radius / t(TILE_WIDTH)
        bb = np.empty((pr.shape[0], 4), np.int64)
        for i in range(2):
            tc = xy[:, i] / t(TILE_WIDTH)
            bb[:, i] = _trunc_clamp(tc - tr, 0, int(tile_bounds[i]))
            bb[:, 2 + i] = _trunc_clamp((tc + tr) + t(1.0), 0, int(tile_bounds[i]))
    return bb


def classify(projected, tile_bounds):
    """Float64 restatement of walk_rect: per visible splat the area (tiles) of the rectangle its walk enumerates and
    whether its reach is unknown (make_tile_reach: det Q * 1024 < q0 * q2, every tile through the late ring).
    Returns (area int64 [V], unknown bool [V]).  Approximate where the device's f32 rounding decides."""
    pr = np.asarray(projected, dtype=np.float64)
    bb = reference_bbox(pr, tile_bounds, np.float64)
    xy = pr[:, 0:2]
    with np.errstate(all="ignore"):
        sigma = np.log(pr[:, 8] * 255.0)
        any_ = sigma > 0.0
        den = 2.0 * sigma
        q0, q1, q2 = pr[:, 2] / den, pr[:, 3] / den, pr[:, 4] / den
        dq = q0 * q2 - q1 * q1
        hx, hy = np.sqrt(q2 / dq), np.sqrt(q0 / dq)
        ok = any_ & (dq > 0) & (q0 > 0) & (q2 > 0) & (dq * 1024.0 >= q0 * q2) & (hx < 3.0e37) & (hy < 3.0e37)
        half = TILE_WIDTH / 2.0
        for i, hh in enumerate((hx, hy)):
            r = hh * 1.001 + (half + 0.02)
            # the slack goes in before the saturating conversion, as in walk_rect
            lo = _trunc_clamp(np.floor((xy[:, i] - r - half) / TILE_WIDTH) - 1.0, -2**31, 2**31)
            hi = _trunc_clamp(np.floor((xy[:, i] + r - half) / TILE_WIDTH) + 2.0, -2**31, 2**31)
            nlo = np.clip(lo, bb[:, i], bb[:, 2 + i])
            nhi = np.maximum(np.clip(hi, bb[:, i], bb[:, 2 + i]), nlo)
            bb[:, i] = np.where(ok, nlo, bb[:, i])
            bb[:, 2 + i] = np.where(ok, nhi, bb[:, 2 + i])
    area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    area = np.where(any_, area, 0)
    return area.astype(np.int64), (any_ & ~ok)


def regime(projected, tile_bounds, n_total):
    """What `classify` says about one frame: V, the class counts, the queue items and the paths they select."""
    V = int(np.asarray(projected).shape[0])
    area, unknown = classify(projected, tile_bounds)
    inline_limit = SMALL_AREA_MANY if V > SMALL_AREA_SWITCH else SMALL_AREA
    queued = area > inline_limit
    items = int(((area[queued] + CHUNK_TILES - 1) // CHUNK_TILES).sum())
    return dict(V=V, n_small=int((area <= SMALL_AREA).sum()), n_mid=int(((area > SMALL_AREA) & (area <= 64)).sum()),
                n_big=int((area > 64).sum()), n_zero=int((area == 0).sum()), n_unknown=int(unknown.sum()),
                n_unknown_queued=int((unknown & queued).sum()), inline_limit=inline_limit, n_queued=int(queued.sum()),
                items=items, capacity=int(n_total), half_wave=V <= HALF_WAVE_SPLATS, flat_emit=V >= FLAT_EMIT_MIN,
                group=4 if items <= GROUP4_MAX else (16 if items <= GROUP16_MAX else 64))


# ---- the cases of tests/test_gpu_binning.py (and of the CPU check of `classify`) ---------------------------------------
# name -> (directed_cloud arguments, w, h, max_intersects).  The counts in the comments are what `regime` gives on the
# oracle's records (CPU); the GPU module asserts the regime each case names from them, with a 20 % margin to every
# item-count threshold.  The V thresholds are exact by construction.

def _v_case(V):
    return dict(cloud=dict(n=V + 1000, seed=11, fr_mid=0.02, fr_big=0.006, fr_thin=0.004, n_hidden=1000),
                w=1024, h=1024, cap=4_000_000)


_BITS_CLOUD = dict(n=60_000, seed=17, fr_mid=0.1, fr_big=0.05, fr_thin=0.02)
_UNKNOWN = dict(seed=19, fr_mid=0.0, fr_big=0.0, fr_thin=1.0, big_sigma=(40, 120), thin_aspect=300)

V_BOUNDARIES = ((1 << 18), (1 << 18) + 1, (1 << 19) - 1, (1 << 19), (1 << 19) + 1)
TILE_BIT_FRAMES = {1: (16, 16), 15: (240, 16), 16: (256, 16), 255: (272, 240), 256: (256, 256), 4095: (1040, 1008),
                   4096: (1024, 1024)}
WIDE_FRAMES = {65535: (4112, 4080), 65536: (4096, 4096), 65792: (4112, 4096), 65552: (65552, 256)}
WIDE_CAPS = (6_000_000, 9_000_000)  # the fused sort shape, and the 3-launch one (> 512 x 16 384 keys)

CASES = {f"v_{V}": _v_case(V) for V in V_BOUNDARIES}
CASES.update({
    "flat_truncated": dict(_v_case((1 << 19) + 1), cap=1_000_003),
    "group16": dict(cloud=dict(n=100_000, seed=13, fr_mid=0.1, fr_big=0.2, fr_thin=0.1), w=1024, h=1024,
                    cap=8_000_000),
    "group64": dict(cloud=dict(n=400_000, seed=13, fr_mid=0.05, fr_big=0.1, fr_thin=0.25), w=1024, h=1024,
                    cap=12_000_000),
    "group64_1080p": dict(cloud=dict(n=400_000, seed=13, fr_mid=0.05, fr_big=0.1, fr_thin=0.25), w=1920, h=1080,
                          cap=12_000_000),
    "group64_queue_overflow": dict(cloud=dict(n=300_000, seed=13, fr_mid=0.05, fr_big=0.3, fr_thin=0.4), w=1024,
                                   h=1024, cap=16_000_000),
    "unknown_queued": dict(cloud=dict(n=220_000, n_hidden=200_000, **_UNKNOWN), w=1024, h=1024, cap=4_000_000),
    "unknown_inline_retest": dict(cloud=dict(n=20_000, **_UNKNOWN), w=1024, h=1024, cap=4_000_000),
})
CASES.update({f"tiles_{t}": dict(cloud=_BITS_CLOUD, w=w, h=h, cap=4_000_000) for t, (w, h) in TILE_BIT_FRAMES.items()})
CASES.update({f"wide_{t}_cap{cap // 1_000_000}m": dict(cloud=_BITS_CLOUD, w=w, h=h, cap=cap)
              for t, (w, h) in WIDE_FRAMES.items() for cap in WIDE_CAPS})


def case_cloud(name):
    c = CASES[name]
    return directed_cloud(w=c["w"], h=c["h"], **c["cloud"])
