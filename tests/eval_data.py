"""Test-written datasets for the evaluation tests (tests/test_eval_cpu.py, tests/test_gpu_eval.py): a NeRF-synthetic
tree (transforms_*.json + PNG frames) and a binary COLMAP model (sparse/0/*.bin + images/), both with known cameras."""
import json
import math
import os
import struct

import numpy as np


def png_bytes(img: np.ndarray) -> bytes:
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    return buf.getvalue()


def noise_image(w, h, channels, seed):
    """Smooth-ish u8 noise: a coarse random grid upsampled, plus fine noise (so the SSIM windows see structure)."""
    rng = np.random.default_rng(seed)
    coarse = rng.random((h // 16 + 2, w // 16 + 2, channels))
    ys, xs = np.arange(h) / 16.0, np.arange(w) / 16.0
    img = coarse[ys.astype(int)][:, xs.astype(int)] * 0.8 + rng.random((h, w, channels)) * 0.2
    return np.clip(img * 255.0, 0, 255).astype(np.uint8)


def look_at_gl(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world 4x4 in the NeRF-synthetic convention (OpenGL camera: looks along -z, y up; world z up)."""
    p, t, u = (np.asarray(v, dtype=np.float64) for v in (position, target, up))
    f = (t - p) / np.linalg.norm(t - p)
    r = np.cross(f, u)
    r /= np.linalg.norm(r)
    u2 = np.cross(r, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u2, -f, p
    return m


def write_nerf(root, w, h, n_train=2, n_val=3, camera_angle_x=0.6911112070083618, with_val=True, seed=0):
    """transforms_train.json (+ transforms_val.json) with n views each on a circle of radius 4 at height 1.
    Returns {"train": [(file_path, c2w, image)], "val": [...], "camera_angle_x": ...}."""
    os.makedirs(root, exist_ok=True)
    out = {"camera_angle_x": camera_angle_x}
    splits = [("train", n_train)] + ([("val", n_val)] if with_val else [])
    for k, (split, n) in enumerate(splits):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames, recs = [], []
        for i in range(n):
            a = 2.0 * math.pi * (i + 0.5 * k) / max(n, 1) + 0.3
            c2w = look_at_gl((4.0 * math.cos(a), 4.0 * math.sin(a), 1.0))
            c2w = c2w.astype(np.float32).astype(np.float64)  # the file holds what an f32 reader sees
            img = noise_image(w, h, 4 if (i % 2) else 3, seed + 31 * k + i)
            rel = f"./{split}/r_{i}"
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(png_bytes(img))
            frames.append({"file_path": rel, "rotation": 0.0, "transform_matrix": c2w.tolist()})
            recs.append((rel, c2w, img))
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": camera_angle_x, "frames": frames}, f)
        out[split] = recs
    return out


def _quat_wxyz_from_mat3(m):
    """Unit quaternion (w, x, y, z) of a proper rotation matrix (Shepperd: the branch of the largest diagonal term)."""
    t = np.trace(m)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2.0
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif m[1, 1] > m[2, 2]:
        s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    return np.array(q)


def write_colmap(root, w, h, n_images=3, fx=380.0, fy=372.0, cx=None, cy=None, seed=0):
    """Binary COLMAP model (PINHOLE camera 1, n images, a few 3-D points) + PNGs under images/.
    Returns {"camera": (w, h, fx, fy, cx, cy), "images": [(name, quat_wxyz, tvec, image)]} with f32-exact poses."""
    cx = w * 0.5 + 3.0 if cx is None else cx
    cy = h * 0.5 - 2.0 if cy is None else cy
    os.makedirs(os.path.join(root, "sparse", "0"), exist_ok=True)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    cb = struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 1, w, h) + struct.pack("<4d", fx, fy, cx, cy)
    ib = struct.pack("<Q", n_images)
    imgs = []
    for i in range(n_images):
        a = 2.0 * math.pi * i / n_images + 0.2
        pos = np.array([4.0 * math.sin(a), 0.4, -4.0 * math.cos(a)])
        # camera +z looks at the origin, +y roughly down (the kernel's frame): columns of camera-to-world
        f = -pos / np.linalg.norm(pos)
        r = np.cross(np.array([0.0, 1.0, 0.0]), f)
        r /= np.linalg.norm(r)
        d = np.cross(f, r)
        r_cw = np.stack([r, d, f], 1)
        r_wc = r_cw.T
        q = _quat_wxyz_from_mat3(r_wc).astype(np.float32).astype(np.float64)
        t = (-r_wc @ pos).astype(np.float32).astype(np.float64)
        name = f"img_{i:02d}.png"
        img = noise_image(w, h, 3, seed + 7 * i)
        with open(os.path.join(root, "images", name), "wb") as fh:
            fh.write(png_bytes(img))
        ib += struct.pack("<i4d3di", i + 1, *q, *t, 1) + name.encode() + b"\0" + struct.pack("<Q", 0)
        imgs.append((name, q, t, img))
    pb = struct.pack("<Q", 2)
    for pid in (1, 2):
        pb += struct.pack("<Q3d3BdQ", pid, 0.1 * pid, -0.2, 0.3, 200, 100, 50, 0.5, 0)
    for nm, b in (("cameras.bin", cb), ("images.bin", ib), ("points3D.bin", pb)):
        with open(os.path.join(root, "sparse", "0", nm), "wb") as fh:
            fh.write(b)
    return {"camera": (w, h, fx, fy, cx, cy), "images": imgs}


def _uniform_dict(w2l, w, h, focal, center, sh_degree):
    return {"viewmat": np.ascontiguousarray(np.asarray(w2l, dtype=np.float32).T).reshape(16),  # column-major
            "focal": np.array(focal, dtype=np.float32), "img_size": np.array([w, h], dtype=np.uint32),
            "tile_bounds": np.array([-(-w // 16), -(-h // 16)], dtype=np.uint32),
            "pixel_center": np.array(center, dtype=np.float32), "sh_degree": int(sh_degree)}


def nerf_uniforms(c2w, camera_angle_x, w, h, sh_degree):
    """Uniforms of a NeRF-synthetic frame built from the JSON per nerf_synthetic.rs:56-88: y and z axes (columns)
    negated, then rotated by +pi/2 about x; the view matrix is the inverse of that camera-to-world."""
    t = np.asarray(c2w, dtype=np.float64).copy()
    t[:, 1] *= -1.0
    t[:, 2] *= -1.0
    rx = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float64)  # from_rotation_x(pi/2)
    t = rx @ t
    f = 0.5 * w / math.tan(0.5 * camera_angle_x)
    fovy = 2.0 * math.atan(h / (2.0 * f))
    return _uniform_dict(np.linalg.inv(t), w, h, (f, 0.5 * h / math.tan(0.5 * fovy)), (0.5 * w, 0.5 * h), sh_degree)


def colmap_uniforms(quat_wxyz, tvec, camera, sh_degree):
    """Uniforms of a COLMAP image per colmap.rs:73-96: COLMAP's (quat, tvec) is world-to-camera, so it IS the view
    matrix (the reader inverts it into the camera pose and the op inverts it back); fov from the focal lengths,
    principal point as a fraction of the size."""
    w, h, fx, fy, cx, cy = camera
    qw, qx, qy, qz = (float(v) for v in quat_wxyz)
    n = math.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw, qx, qy, qz = qw / n, qx / n, qy / n, qz / n
    r = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                  [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                  [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = r, np.asarray(tvec, dtype=np.float64)
    return _uniform_dict(w2c, w, h, (fx, fy), (cx, cy), sh_degree)


def uniforms_close(got, want, atol=1e-6):
    """The fields eval builds from a camera: viewmat and focal / pixel centre (relative for the pixel-sized ones)."""
    assert list(got["img_size"]) == list(want["img_size"])
    assert np.abs(np.asarray(got["viewmat"], np.float64) - want["viewmat"]).max() <= atol, (got["viewmat"],
                                                                                           want["viewmat"])
    for k in ("focal", "pixel_center"):
        g, e = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert np.abs(g - e).max() <= atol * np.abs(e).max(), (k, g, e)
