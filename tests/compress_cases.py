"""Directed inputs of the compressed-splat tests, each on the smallest count at which its piece can go wrong.  A case is
a dict of the five float32 arrays of a cloud in the Splats layout (means [N,3], log_scales [N,3], rotation [N,4],
raw_opacity [N], sh_coeffs [N,(d+1)^2,3]); CASES maps a name to a function that builds it from fixed seeds."""
import numpy as np

F = np.float32


def cloud(n, sh_degree, seed):
    """A seeded cloud: means in a box of different extents per axis, log-scales around -3, random rotations, raw
    opacities in (-6, 6), DC colours in (-2, 2) and higher bands in (-1.5, 1.5)."""
    rng = np.random.default_rng(seed)
    coeffs = (sh_degree + 1) ** 2
    sh = rng.uniform(-1.5, 1.5, (n, coeffs, 3))
    sh[:, 0, :] = rng.uniform(-2.0, 2.0, (n, 3))
    return {"means": (rng.uniform(-1.0, 1.0, (n, 3)) * [4.0, 1.0, 2.5]).astype(F),
            "log_scales": rng.normal(-3.0, 1.0, (n, 3)).astype(F),
            "rotation": rng.normal(0.0, 1.0, (n, 4)).astype(F),
            "raw_opacity": rng.uniform(-6.0, 6.0, n).astype(F),
            "sh_coeffs": sh.astype(F)}


def _equal_means():
    c = cloud(300, 0, 21)
    c["means"][:] = F([0.25, -1.5, 3.0])  # every key ties: the order is the identity
    return c


def _flat_axis():
    c = cloud(300, 0, 22)
    c["means"][:, 2] = F(0.75)  # zero extent in z: q_z = 0, min_z == max_z in every chunk
    return c


def _tiny_extent():
    """Every chunk's extent in scale_x, in red and in the y mean is below 1e-5 with values strictly inside it, so
    that norm's third branch decides."""
    c = cloud(300, 1, 23)
    rng = np.random.default_rng(24)
    c["log_scales"][:, 0] = (F(-2.0) + rng.integers(0, 20, 300) * F(2.0 ** -22)).astype(F)
    c["sh_coeffs"][:, 0, 0] = (F(0.5) + rng.integers(0, 8, 300) * F(2.0 ** -21)).astype(F)
    c["means"][:, 1] = (F(1.0) + rng.integers(0, 16, 300) * F(2.0 ** -21)).astype(F)
    return c


def _quaternions():
    quats = []
    for big in range(4):
        for sign in (1.0, -1.0):
            q = [0.2, -0.3, 0.25, 0.1]
            q[big] = 0.9 * sign
            quats.append(q)
    for sw in (1.0, -1.0):
        for sx in (1.0, -1.0):
            quats.append([0.6 * sw, 0.6 * sx, 0.3, -0.2])  # |w| = |x| exactly: the first index wins
    quats += [[0.5, 0.5, 0.5, 0.5], [-0.5, 0.5, -0.5, 0.5], [0.1, -0.7, 0.2, 0.7], [0.0, 0.3, -0.3, 0.3]]
    quats += [[5.0, -1.0, 2.0, 0.5], [1e-3, 2e-3, -3e-3, 1e-3], [1e-20, 2e-20, 0.0, -1e-20]]  # not normalised
    quats += [[0.0, 0.0, 0.0, 0.0], [-0.0, 0.0, -0.0, 0.0], [1e30, 1e30, 0.0, 0.0], [1e-30, 0.0, 0.0, 1e-30]]  # identity
    quats += [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -1.0], [0.0, -0.0, 1.0, 0.0]]
    c = cloud(len(quats), 0, 25)
    c["rotation"] = np.asarray(quats, dtype=F)
    return c


def _ranges():
    c = cloud(300, 3, 26)
    c["log_scales"][:8] = F([[-25.0, -20.0, 20.0], [25.0, 20.0, -20.0], [-20.000002, 19.999998, 0.0],
                             [30.0, -30.0, 21.0], [-3.0, -3.0, -3.0], [1e4, -1e4, 0.0], [20.000002, -19.999998, 5.0],
                             [-21.0, 21.0, -19.0]])
    c["raw_opacity"][:6] = F([30.0, -30.0, 0.0, -0.0, 88.0, -104.0])
    edge = F([-4.0, 4.0, -4.5, 5.0, np.nextafter(F(4.0), F(0.0)), np.nextafter(F(-4.0), F(-5.0)), -0.0, 3.984375,
              -3.984375, 100.0, -100.0, 0.015625])
    c["sh_coeffs"][:12, 1:, :] = edge[:, None, None]
    c["sh_coeffs"][12:24, 3, 1] = edge
    c["means"][0] = F([-0.0, 0.0, -0.0])
    c["means"][1] = F([0.0, -0.0, 0.0])
    c["means"][2, 0] = F(-0.0)
    return c


def _signed_zero_means():
    """All means are +0 or -0: after v + 0.0f every key ties and the bounds are +0, so the order is the identity."""
    c = cloud(40, 0, 27)
    rng = np.random.default_rng(28)
    c["means"] = np.where(rng.random((40, 3)) < 0.5, F(0.0), F(-0.0)).astype(F)
    return c


def _nan():
    c = cloud(10, 1, 29)
    c["sh_coeffs"][7, 2, 1] = F(np.nan)
    return c


CASES = {
    "n1": lambda: cloud(1, 0, 1),
    "n255": lambda: cloud(255, 1, 2),
    "n256": lambda: cloud(256, 1, 3),
    "n257": lambda: cloud(257, 1, 4),  # a last chunk of one row
    "n1000_d0": lambda: cloud(1000, 0, 5),
    "n1000_d1": lambda: cloud(1000, 1, 6),
    "n1000_d2": lambda: cloud(1000, 2, 7),
    "n1000_d3": lambda: cloud(1000, 3, 8),
    "equal_means": _equal_means,
    "flat_axis": _flat_axis,
    "tiny_extent": _tiny_extent,
    "quaternions": _quaternions,
    "ranges": _ranges,
    "signed_zero_means": _signed_zero_means,
}
NAN_CASE = _nan
FIELDS = ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")
