"""General cameras for the depth, antialias and pose tests, and the rigid move that brings a scene built for the
reference test camera in front of one of them.

At the reference test camera the world-to-camera rotation W is the identity: row 2 of W equals column 2, T = J W equals
J W^T, and a gradient pushed through W^T instead of W is unchanged.  Every camera here has a W that is not symmetric.
A case is given by its world-to-camera rotation (axis, angle) and either the world-to-camera translation or the camera's
position; `general` and `free` also move the principal point off the centre and scale fov_y, so that the two focal
lengths differ.

`co_moved` keeps the camera-space geometry of a scene (the visible set, the tile lists and every threshold decision stay
where the existing gates were built) while W becomes general.  The SH coefficients are not rotated: above degree 0 the
moved scene has other colours, which no test here minds.  `free` is the one camera meant to be used WITHOUT the move."""
import math

import numpy as np

from tests import helpers as H

REFERENCE = "reference"
CASES = {
    # 0.6 rad about one axis: tilt_x / tilt_y make row 2 of W differ from column 2, roll_z leaves row 2 at (0, 0, 1)
    # and mixes x and y only
    "tilt_x": dict(axis=(1.0, 0.0, 0.0), angle=0.6, t=(0.3, -0.2, 0.9)),
    "tilt_y": dict(axis=(0.0, 1.0, 0.0), angle=0.6, t=(-0.5, 0.25, 0.6)),
    "roll_z": dict(axis=(0.0, 0.0, 1.0), angle=0.6, t=(0.2, 0.6, -0.4)),
    "general": dict(axis=(0.3, -0.8, 0.5), angle=0.9, t=(0.7, -0.4, 1.3), center_uv=(0.43, 0.58), fov_y_scale=1.1),
    # the quaternion's w is near 0 (cos 1.5 = 0.07)
    "near_half_turn": dict(axis=(0.5, 0.4, -0.77), angle=3.0, t=(-0.6, 0.8, 1.1)),
    # not co-moved: the geometry changes too
    "free": dict(axis=(0.3, -0.8, 0.5), angle=0.9, position=(1.5, -0.7, -6.0), center_uv=(0.43, 0.58),
                 fov_y_scale=1.1),
}
CO_MOVED = tuple(k for k in CASES if k != "free")
ALL = tuple(CASES)


def rotation64(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`, float64 [3,3]."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def _f32(v):
    return [float(np.float32(x)) for x in v]


def camera_args(name, w, h, base=None):
    """brush_amd.Camera / oracle.make_uniforms arguments of a case: dict(position, rotation_xyzw, fov_x, fov_y,
    center_uv).  `base` gives the fields of view the case starts from (default: the reference test camera's).  Position
    and quaternion are rounded to f32 here, so that everything built from them starts from the same numbers."""
    base = dict(H.reference_test_camera(w, h) if base is None else base)
    if name == REFERENCE:
        return dict(position=_f32(base["position"]), rotation_xyzw=_f32(base["rotation_xyzw"]), fov_x=base["fov_x"],
                    fov_y=base["fov_y"], center_uv=tuple(base["center_uv"]))
    c = CASES[name]
    a = np.asarray(c["axis"], np.float64)
    a = a / np.linalg.norm(a)
    # the camera's local-to-world rotation is the inverse of W: the same axis, the opposite angle
    s, co = math.sin(-0.5 * c["angle"]), math.cos(-0.5 * c["angle"])
    if "position" in c:
        pos = np.asarray(c["position"], np.float64)
    else:
        pos = -rotation64(c["axis"], c["angle"]).T @ np.asarray(c["t"], np.float64)
    return dict(position=_f32(pos), rotation_xyzw=_f32([a[0] * s, a[1] * s, a[2] * s, co]), fov_x=base["fov_x"],
                fov_y=base["fov_y"] * c.get("fov_y_scale", 1.0), center_uv=tuple(c.get("center_uv", (0.5, 0.5))))


def camera(name, w, h, base=None):
    import brush_amd

    c = camera_args(name, w, h, base)
    return brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def _mat3_xyzw(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def matrix64(name, w=64, h=64, base=None):
    """The world-to-camera matrix the kernels are given, [4,4] float64 holding f32 values: the inverse of the
    local-to-world matrix of the f32 position and quaternion, rounded to f32 (camera.py, oracle.make_uniforms)."""
    c = camera_args(name, w, h, base)
    l2w = np.eye(4)
    l2w[:3, :3] = _mat3_xyzw(c["rotation_xyzw"])
    l2w[:3, 3] = c["position"]
    return np.linalg.inv(l2w).astype(np.float32).astype(np.float64)


def is_symmetric(name):
    """True where W = W^T to f32 rounding: there a W / W^T mix-up cannot show."""
    W = matrix64(name)[:3, :3]
    return bool(np.abs(W - W.T).max() <= 1e-6)


def quat_wxyz_of(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, by the branch with the largest pivot (safe near a half
    turn)."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = [tr, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(cand))
    if k == 0:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2 * R[0, 0] - tr, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2 * R[1, 1] - tr, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2 * R[2, 2] - tr])
    return q / np.linalg.norm(q)


def quat_mul_wxyz(a, b):
    """Hamilton product a (x) b, (w, x, y, z); a [4], b [N,4]."""
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = (b[:, i] for i in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def co_moved(cloud, w, h, cam, m_ref=None):
    """The cloud (built for the reference test camera of a w x h frame, or for the camera whose float64 world-to-camera
    matrix is `m_ref`) moved rigidly by G = M_cam^-1 M_ref in float64: camera `cam` sees it where the reference camera
    saw the original, up to the f32 rounding of the moved means and quaternions."""
    if cam == REFERENCE:
        return dict(cloud)
    if m_ref is None:
        m_ref = matrix64(REFERENCE, w, h)
    G = np.linalg.inv(matrix64(cam, w, h)) @ np.asarray(m_ref, np.float64)
    out = dict(cloud)
    out["means"] = (np.asarray(cloud["means"], np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    out["quats"] = quat_mul_wxyz(quat_wxyz_of(G[:3, :3]), np.asarray(cloud["quats"], np.float64)).astype(np.float32)
    return out


# ---- the scenes the GPU tests run, with the conditions that keep them meaningful asserted from the oracle
GPU_SCENES = tuple((kind, name) for kind in ("tiny_case", "basic_case") for name in CO_MOVED) + \
    (("ragged", "general"), ("ragged", "near_half_turn"), ("ragged", "free"))
MAX_FLIP_FRACTION = 1e-3  # test_gpu_antialias.py's cap on the share of pixels the oracle flags flip_risk
FREE_MIN_VISIBLE = 1000


def oracle_uniforms(name, w, h, sh_degree, base=None):
    from oracle import oracle as O

    a = camera_args(name, w, h, base)
    return O.make_uniforms(a["position"], a["rotation_xyzw"], a["fov_x"], a["fov_y"], a["center_uv"], (w, h), sh_degree)


def _oracle_counts(u, cloud):
    from oracle import oracle as O

    _, aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"])
    return (int(aux["num_visible"][0]), int(aux["num_intersections"][0]),
            float(aux["flip_risk"].astype(bool).mean()))


_scene_cache = {}


def scene_at(kind, name, normalised=False):
    """(cloud, w, h, facts) of test_gpu_depth's scene `kind` for camera `name`: co-moved unless the camera is `free`.
    `normalised`: the quaternions normalised in f32 first (test_gpu_pose's scenes).  Asserted from the CPU oracle, so
    that no test goes green on an empty or a different frame: a co-moved scene keeps the visible and the intersection
    count of its original seen from the reference pose through the same lens (the case's principal point and fields of
    view); `free` sees at least FREE_MIN_VISIBLE splats; at most MAX_FLIP_FRACTION of the pixels are flip-risk."""
    key = (kind, name, normalised)
    if key in _scene_cache:
        return _scene_cache[key]
    from brush_amd.render import sh_degree_from_coeffs
    from tests import test_gpu_depth as TD

    cloud, w, h = TD._scene(kind)
    cloud = dict(cloud)
    if normalised:
        q = np.asarray(cloud["quats"], np.float32)
        cloud["quats"] = (q / np.sqrt((q * q).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    deg = sh_degree_from_coeffs(cloud["sh"].shape[1])
    u = oracle_uniforms(name, w, h, deg)
    if name == "free":
        moved = cloud
        V, I, risk = _oracle_counts(u, moved)
        assert V >= FREE_MIN_VISIBLE, (kind, name, V)
    else:
        moved = co_moved(cloud, w, h, name)
        V, I, risk = _oracle_counts(u, moved)
        u0 = dict(oracle_uniforms(REFERENCE, w, h, deg))
        u0["focal"], u0["pixel_center"] = u["focal"], u["pixel_center"]
        V0, I0, _ = _oracle_counts(u0, cloud)
        assert (V, I) == (V0, I0) and V > 0, (kind, name, V, I, V0, I0)
    assert risk <= MAX_FLIP_FRACTION, (kind, name, risk)
    _scene_cache[key] = (moved, w, h, dict(visible=V, intersections=I, flip_risk=risk))
    return _scene_cache[key]
