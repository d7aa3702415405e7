"""Host references of the undistortion (brush_amd/csrc/undistort.hip), written from the definition and not imported
from the package: a NumPy float32 restatement that the kernels must equal bit for bit (every operation on float32 arrays,
one rounding each, in the definition's order), and a float64 evaluation of the same camera model for the geometry.

A map is a dict of the sixteen numbers fx fy cx cy iofx iofy ocx ocy k1..k6 p1 p2; `make_map` builds one the way the
host code does (the inverse focal divided in float32)."""
import numpy as np

F = np.float32
COEFFS = ("k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2")
FIELDS = ("fx", "fy", "cx", "cy", "iofx", "iofy", "ocx", "ocy") + COEFFS


def make_map(fx, fy, cx, cy, ofx, ofy, ocx, ocy, **coeffs):
    """Source camera (fx, fy, cx, cy), output camera (ofx, ofy, ocx, ocy), coefficients by name (missing: 0)."""
    assert set(coeffs) <= set(COEFFS)
    m = {"fx": fx, "fy": fy, "cx": cx, "cy": cy, "ocx": ocx, "ocy": ocy,
         "iofx": float(F(1.0) / F(ofx)), "iofy": float(F(1.0) / F(ofy))}
    m.update({k: float(coeffs.get(k, 0.0)) for k in COEFFS})
    return {k: float(F(m[k])) for k in FIELDS}  # what a struct of floats holds


def q8_f32(m, w, h, ow, oh):
    """(qx, qy, valid) of every output pixel, [oh, ow]: the float32 recipe, then rint to Q8."""
    c = {k: F(v) for k, v in m.items()}
    X = np.broadcast_to(np.arange(ow, dtype=np.int64).astype(F)[None, :], (oh, ow))
    Y = np.broadcast_to(np.arange(oh, dtype=np.int64).astype(F)[:, None], (oh, ow))
    half, one, two = F(0.5), F(1.0), F(2.0)
    with np.errstate(all="ignore"):
        x = ((X + half) - c["ocx"]) * c["iofx"]
        y = ((Y + half) - c["ocy"]) * c["iofy"]
        r2 = x * x + y * y
        num = one + r2 * (c["k1"] + r2 * (c["k2"] + r2 * c["k3"]))
        den = one + r2 * (c["k4"] + r2 * (c["k5"] + r2 * c["k6"]))
        rad = num / den
        a = x * y
        xd = x * rad + ((two * c["p1"]) * a + c["p2"] * (r2 + (two * x) * x))
        yd = y * rad + (c["p1"] * (r2 + (two * y) * y) + (two * c["p2"]) * a)
        u = (c["fx"] * xd + c["cx"]) - half
        v = (c["fy"] * yd + c["cy"]) - half
        ru, rv = np.rint(u * F(256.0)), np.rint(v * F(256.0))
        for t in (x, r2, rad, xd, u, ru):
            assert t.dtype == np.float32
        finite = (np.abs(ru) < F(2.0 ** 30)) & (np.abs(rv) < F(2.0 ** 30))  # False for NaN
    qx = np.where(finite, ru, F(-1.0)).astype(np.int64)
    qy = np.where(finite, rv, F(-1.0)).astype(np.int64)
    valid = finite & (qx >= 0) & (qx <= (w - 1) * 256) & (qy >= 0) & (qy <= (h - 1) * 256)
    return qx, qy, valid


def distort_f64(m, px, py):
    """The camera model in float64: output pixel coordinates (centres at +0.5) -> source pixel coordinates.  Uses the
    map's float32 fields as given (so 1 / iofx is the output focal the kernel sees)."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    x, y = (px - m["ocx"]) * m["iofx"], (py - m["ocy"]) * m["iofy"]
    r2 = x * x + y * y
    with np.errstate(all="ignore"):
        rad = (1 + r2 * (m["k1"] + r2 * (m["k2"] + r2 * m["k3"]))) / (1 + r2 * (m["k4"] + r2 * (m["k5"] + r2 * m["k6"])))
        a = x * y
        xd = x * rad + (2 * m["p1"] * a + m["p2"] * (r2 + 2 * x * x))
        yd = y * rad + (m["p1"] * (r2 + 2 * y * y) + 2 * m["p2"] * a)
        return m["fx"] * xd + m["cx"], m["fy"] * yd + m["cy"]


def q8_f64(m, ow, oh):
    """The float64 model's Q8 source index coordinates (unrounded floats) of every output pixel centre."""
    px, py = np.meshgrid(np.arange(ow) + 0.5, np.arange(oh) + 0.5)
    u, v = distort_f64(m, px, py)
    return (u - 0.5) * 256.0, (v - 0.5) * 256.0


def undistort_u8_ref(img, m, ow, oh):
    """(dst uint8 [oh,ow,c], valid uint8 [oh,ow]) of a uint8 [h,w,c] image."""
    h, w, _ = img.shape
    qx, qy, valid = q8_f32(m, w, h, ow, oh)
    qx, qy = np.where(valid, qx, 0), np.where(valid, qy, 0)
    x0, ax, y0, ay = qx >> 8, qx & 255, qy >> 8, qy & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = img.astype(np.int64)
    acc = (((256 - ax) * (256 - ay))[..., None] * s[y0, x0] + (ax * (256 - ay))[..., None] * s[y0, x1]
           + ((256 - ax) * ay)[..., None] * s[y1, x0] + (ax * ay)[..., None] * s[y1, x1])
    assert acc.max(initial=0) + 32768 < 1 << 24
    out = (acc + 32768) >> 16
    out[~valid] = 0
    return out.astype(np.uint8), valid.astype(np.uint8)


def undistort_nearest_ref(a, m, ow, oh):
    """A [h,w] array of any dtype: the nearest element, copied (bits kept); 0 where invalid."""
    h, w = a.shape
    qx, qy, valid = q8_f32(m, w, h, ow, oh)
    sx = np.clip((np.where(valid, qx, 0) + 128) >> 8, 0, w - 1)
    sy = np.clip((np.where(valid, qy, 0) + 128) >> 8, 0, h - 1)
    out = a[sy, sx].copy()
    out[~valid] = 0
    return out


# ---------------------------------------------------------------------------- a tiny COLMAP tree
def pattern_image(w, h, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def write_colmap_tree(root, cameras, w=48, h=36):
    """A text-format COLMAP tree under `root`: camera i + 1 is cameras[i] = (model name, params), image i + 1 (im{i}.png,
    w x h RGB, seeded) is taken with it.  Returns the images as arrays."""
    import os

    from PIL import Image

    os.makedirs(os.path.join(root, "sparse", "0"))
    os.makedirs(os.path.join(root, "images"))
    images = []
    with open(os.path.join(root, "sparse", "0", "cameras.txt"), "w") as f:
        for i, (model, params) in enumerate(cameras):
            f.write(f"{i + 1} {model} {w} {h} " + " ".join(repr(float(p)) for p in params) + "\n")
    with open(os.path.join(root, "sparse", "0", "images.txt"), "w") as f:
        for i in range(len(cameras)):
            f.write(f"{i + 1} 1.0 0.0 0.0 0.0 {0.1 * i} 0.0 4.0 {i + 1} im{i}.png\n\n")
            images.append(pattern_image(w, h, 3, 40 + i))
            Image.fromarray(images[-1]).save(os.path.join(root, "images", f"im{i}.png"))
    return images


# ---------------------------------------------------------------------------- the directed cases of the GPU tests
# Every model with fx != fy and an off-centre principal point; coefficient sets: strong barrel, pincushion, tangential
# terms of a few 1e-2, a rational FULL_OPENCV set.
PARAMS = {
    "simple_radial_barrel": {"k1": -0.3},
    "simple_radial_pincushion": {"k1": 0.2},
    "radial": {"k1": -0.3, "k2": 0.08},
    "opencv_tangential": {"k1": -0.12, "k2": 0.03, "p1": 0.03, "p2": -0.02},
    "full_opencv_rational": {"k1": 0.3, "k2": -0.1, "p1": 0.01, "p2": -0.015, "k3": 0.02, "k4": 0.35, "k5": -0.05,
                             "k6": 0.01},
}
# (w, h) of the source -> (ow, oh) of the output
SHAPES = [((1, 1), (1, 1)), ((17, 13), (17, 13)), ((64, 64), (64, 64)), ((65, 9), (65, 9)), ((257, 5), (257, 5)),
          ((64, 48), (80, 33)), ((40, 50), (23, 61))]
SCALES = (1.0, 0.25, 2.0)


def case_map(w, h, ow, oh, params, scale=1.0):
    """A source camera of about 70 degrees across the longer side, fx != fy, principal point off the centre, seen by an
    output camera of focal scale * (fx, fy) whose principal point sits at the same fraction of its own size."""
    f = 0.7 * max(w, h)
    fx, fy = f, 1.07 * f
    cx, cy = 0.47 * w + 0.3, 0.54 * h - 0.2
    return make_map(fx, fy, cx, cy, scale * fx * ow / w, scale * fy * oh / h, cx * ow / w, cy * oh / h, **params)


def all_cases():
    """(name, w, h, ow, oh, map): every shape with every parameter set at scale 1, and every parameter set at the
    scales 0.25 and 2 on two of the shapes."""
    out = []
    for (w, h), (ow, oh) in SHAPES:
        for pname, params in PARAMS.items():
            out.append((f"{w}x{h}->{ow}x{oh} {pname}", w, h, ow, oh, case_map(w, h, ow, oh, params)))
    for scale in SCALES[1:]:
        for (w, h), (ow, oh) in (SHAPES[2], SHAPES[5]):
            for pname, params in PARAMS.items():
                out.append((f"{w}x{h}->{ow}x{oh} {pname} scale {scale}", w, h, ow, oh,
                            case_map(w, h, ow, oh, params, scale)))
    return out
