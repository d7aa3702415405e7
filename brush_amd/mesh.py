"""Export a trained scene as a triangle mesh: render depth from the dataset's views, fuse it into a TSDF volume, extract
the surface (brush_amd/tsdf.py).

    python -m brush_amd.mesh SPLATS DATASET [--resolution 256 | --voxel-size S] [--bounds x0,y0,z0,x1,y1,z1]
                             [--trunc-voxels 4] [--alpha-min 0.5] [--max-depth D] [--min-views 2]
                             [--views train|eval|all] [--antialiased] [--no-undistort] [--no-masks]
                             [--depth expected|median] [--median-level 0.5]
                             [--export OUT.ply] [--json OUT.json]
                             [--format auto|nerf|colmap] [--eval-split-every K] [--max-resolution R]

Without --bounds the grid encloses the central 98 % of the splats whose opacity is at least 0.1 (default_bounds), padded
by 5 % of its longest side.  Prints the grid and its size in bytes, the number of views fused, the fraction of voxels
any view observed, and the vertex and face counts; --export writes a binary PLY with per-vertex colours.
--depth median fuses the median depth (brush_amd/median_depth.py) instead of the expected depth D / alpha: no skirts at
silhouettes, thin structures survive.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import cli


@dataclass
class Mesh:
    """An indexed triangle mesh on the host."""
    vertices: np.ndarray  # float32 [V, 3]
    colors: np.ndarray    # uint8 [V, 3]
    faces: np.ndarray     # int32 [F, 3], counter-clockwise seen from outside


_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def mesh_to_ply(mesh: Mesh) -> bytes:
    """Binary little-endian PLY: element vertex with x y z (float) red green blue (uchar), element face with
    vertex_indices as a list of int with a uchar count."""
    v = np.asarray(mesh.vertices, dtype=np.float32).reshape(-1, 3)
    c = np.asarray(mesh.colors, dtype=np.uint8).reshape(-1, 3)
    f = np.asarray(mesh.faces, dtype=np.int32).reshape(-1, 3)
    if len(c) != len(v):
        raise ValueError(f"{len(v)} vertices need {len(v)} colours, got {len(c)}")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("a face index lies outside the vertices")
    header = ("ply\nformat binary_little_endian 1.0\ncomment brush_amd mesh export\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    vert = np.empty(len(v), dtype=_VERTEX)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=_FACE)
    face["n"], face["v"] = 3, f
    return header.encode("ascii") + vert.tobytes() + face.tobytes()


def mesh_from_ply(data) -> Mesh:
    """Reads what mesh_to_ply writes (a path or bytes); ValueError for any other PLY."""
    if not isinstance(data, (bytes, bytearray)):
        with open(data, "rb") as f:
            data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("only binary little-endian PLY meshes are read")
    elements, props = [], {}
    for line in lines:
        tok = line.split()
        if tok[:1] == ["element"]:
            elements.append((tok[1], int(tok[2])))
            props[tok[1]] = []
        elif tok[:1] == ["property"]:
            props[elements[-1][0]].append(" ".join(tok[1:]))
    want = {"vertex": ["float x", "float y", "float z", "uchar red", "uchar green", "uchar blue"],
            "face": ["list uchar int vertex_indices"]}
    if [e[0] for e in elements] != ["vertex", "face"] or props != want:
        raise ValueError("the PLY does not have the layout mesh_to_ply writes")
    nv, nf = elements[0][1], elements[1][1]
    if len(body) != nv * _VERTEX.itemsize + nf * _FACE.itemsize:
        raise ValueError("the PLY body does not match its header")
    vert = np.frombuffer(body, dtype=_VERTEX, count=nv)
    face = np.frombuffer(body, dtype=_FACE, count=nf, offset=nv * _VERTEX.itemsize)
    if nf and not (face["n"] == 3).all():
        raise ValueError("only triangles are read")
    return Mesh(np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32).reshape(nv, 3),
                np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8).reshape(nv, 3),
                np.array(face["v"], dtype=np.int32).reshape(nf, 3))


def default_bounds(splats, *, opacity_min: float = 0.1, quantiles=(0.01, 0.99), pad: float = 0.05):
    """(lo [3], hi [3]), float64: per axis the `quantiles` of the means of the splats whose opacity (sigmoid of the raw
    one) is at least `opacity_min`, widened on every side by `pad` times the longest side.  ValueError when no splat
    qualifies."""
    lo_q, hi_q = float(quantiles[0]), float(quantiles[1])
    if not 0.0 <= lo_q < hi_q <= 1.0:
        raise ValueError(f"quantiles must satisfy 0 <= lo < hi <= 1, got {quantiles!r}")
    if not (math.isfinite(pad) and pad >= 0):
        raise ValueError(f"pad must be finite and >= 0, got {pad!r}")
    means = splats.means.detach().cpu().numpy().astype(np.float64)
    raw = splats.raw_opacity.detach().cpu().numpy().astype(np.float64).reshape(-1)
    keep = (1.0 / (1.0 + np.exp(-raw)) >= opacity_min) & np.isfinite(means).all(1)
    if not keep.any():
        raise ValueError(f"no splat has an opacity of at least {opacity_min}")
    lo, hi = np.quantile(means[keep], lo_q, axis=0), np.quantile(means[keep], hi_q, axis=0)
    margin = pad * float((hi - lo).max())
    return lo - margin, hi + margin


def grid_for(bounds, *, voxel_size=None, resolution=None):
    """(origin, voxel_size, (nx, ny, nz)) of the grid that covers `bounds` = (lo, hi): with `resolution` R the longest
    side has R voxels, with `voxel_size` the voxel is given; the other sides take as many voxels as cover them.
    ValueError when the grid is over the volume's limits (the message names the limit)."""
    from .tsdf import check_grid

    if (voxel_size is None) == (resolution is None):
        raise ValueError("give exactly one of voxel_size and resolution")
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"bounds must be finite with hi > lo on every axis, got {lo.tolist()} .. {hi.tolist()}")
    extent = hi - lo
    if resolution is not None:
        if int(resolution) != resolution or int(resolution) < 1:
            raise ValueError(f"resolution must be a positive integer, got {resolution!r}")
        voxel_size = float(extent.max()) / int(resolution)
    voxel_size = float(voxel_size)
    if not (math.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size!r}")
    # (the 1e-9 keeps a side that is a whole number of voxels from gaining one through the division's rounding)
    dims = tuple(max(1, int(math.ceil(e / voxel_size - 1e-9))) for e in extent)
    voxel_size, dims = check_grid(voxel_size, dims)
    return tuple(float(x) for x in lo), voxel_size, dims


# ---------------------------------------------------------------------------- command line
def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.mesh",
                                description="fuse a splat file's rendered depth into a TSDF and export a triangle mesh")
    p.add_argument("splats", help=".ply or .safetensors splat file")
    p.add_argument("dataset", help="dataset directory or .zip (NeRF-synthetic or COLMAP): the views to fuse")
    p.add_argument("--resolution", type=int, default=None, metavar="R",
                   help="voxels on the longest side of the grid (default 256)")
    p.add_argument("--voxel-size", type=float, default=None, metavar="S", help="instead: the voxel's side")
    p.add_argument("--bounds", default=None, metavar="x0,y0,z0,x1,y1,z1",
                   help="the box to mesh (default: default_bounds of the splats)")
    p.add_argument("--trunc-voxels", type=float, default=4.0, help="the truncation length in voxels (at least sqrt 3)")
    p.add_argument("--alpha-min", type=float, default=0.5, help="use pixels whose rendered alpha is at least this")
    p.add_argument("--max-depth", type=float, default=None, metavar="D", help="ignore pixels deeper than this")
    p.add_argument("--min-views", type=int, default=2, help="mesh only voxels that at least this many views observed")
    cli.add_views_option(p, "train", "the views to fuse")
    cli.add_antialiased_option(p)
    p.add_argument("--no-masks", action="store_true", help="ignore the dataset's loss masks")
    p.add_argument("--depth", choices=("expected", "median"), default="expected",
                   help="the depth to fuse: the expected depth D / alpha, or the median depth (the splat at which the "
                        "accumulated opacity first reaches --median-level)")
    p.add_argument("--median-level", type=float, default=0.5, metavar="L",
                   help="--depth median: the accumulated opacity at which the depth is taken, 0 < L < 1")
    p.add_argument("--export", default=None, metavar="OUT.ply", help="write the mesh to this .ply")
    cli.add_json_option(p, metavar="OUT.json")
    cli.add_dataset_options(p)
    return p


def parse_bounds(text: str):
    """'x0,y0,z0,x1,y1,z1' -> (lo, hi); ValueError otherwise."""
    try:
        x = [float(t) for t in text.split(",")]
    except ValueError:
        x = []
    if len(x) != 6 or not all(math.isfinite(t) for t in x) or not all(x[a + 3] > x[a] for a in range(3)):
        raise ValueError(f"--bounds takes x0,y0,z0,x1,y1,z1 with x1 > x0, y1 > y0, z1 > z0, got {text!r}")
    return np.array(x[:3]), np.array(x[3:])


def plan_from_args(args) -> dict:
    """What the command line fixes before any file is read: the grid keywords, the bounds if given (and then the grid
    itself, so that one over the limits is refused at once), the fusion and extraction parameters.  ValueError for
    anything out of range."""
    if args.resolution is not None and args.voxel_size is not None:
        raise ValueError("--resolution and --voxel-size are two ways to size the grid: give one of them")
    if args.voxel_size is not None:
        grid_kw = {"voxel_size": args.voxel_size}
    else:
        grid_kw = {"resolution": 256 if args.resolution is None else args.resolution}
    if not (math.isfinite(args.trunc_voxels) and args.trunc_voxels >= math.sqrt(3.0)):
        raise ValueError(f"--trunc-voxels must be at least sqrt(3) = 1.733, got {args.trunc_voxels}")
    if not (math.isfinite(args.alpha_min) and 0.0 < args.alpha_min <= 1.0):
        raise ValueError(f"--alpha-min must be in (0, 1], got {args.alpha_min}")
    if args.max_depth is not None and not args.max_depth > 0:
        raise ValueError(f"--max-depth must be > 0, got {args.max_depth}")
    if args.min_views < 1:
        raise ValueError(f"--min-views must be at least 1, got {args.min_views}")
    if not (math.isfinite(args.median_level) and 0.0 < args.median_level < 1.0):
        raise ValueError(f"--median-level must be finite with 0 < L < 1, got {args.median_level}")
    plan = {"grid_kw": grid_kw, "bounds": None, "grid": None}
    if args.bounds is not None:
        plan["bounds"] = parse_bounds(args.bounds)
        plan["grid"] = grid_for(plan["bounds"], **grid_kw)
    return plan


def main(argv=None) -> int:
    import os

    p = parser()
    args = p.parse_args(argv)
    try:
        plan = plan_from_args(args)
    except ValueError as e:
        p.error(str(e))
    got = cli.dataset_views(args, args.views)  # host work and the refusals first
    if got is None:
        return 2
    from .tsdf import TsdfVolume

    _, views, dev = got
    splats = cli.load_splats(args.splats, dev)
    grid = plan["grid"]
    if grid is None:
        try:
            grid = grid_for(default_bounds(splats), **plan["grid_kw"])
        except ValueError as e:
            p.error(str(e))
    origin, voxel, dims = grid
    vol = TsdfVolume(origin, voxel, dims, trunc=args.trunc_voxels * voxel, device=dev)
    print(f"grid\t{dims[0]} x {dims[1]} x {dims[2]}\tvoxel {voxel:g}\torigin {origin[0]:g},{origin[1]:g},{origin[2]:g}"
          f"\t{vol.nbytes} bytes")
    vol.integrate_splats(splats, views, antialiased=args.antialiased, use_masks=not args.no_masks,
                         alpha_min=args.alpha_min, max_depth=args.max_depth, depth=args.depth,
                         level=args.median_level)
    observed = float((vol.state[0] != 0).float().mean())
    mesh = vol.extract_mesh(args.min_views)
    nv, nf = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    print(f"views\t{len(views)} {args.views}")
    print(f"observed\t{observed:.4f}")
    print(f"mesh\tV {nv}\tF {nf}")
    if args.export:
        with open(args.export, "wb") as f:
            f.write(mesh_to_ply(mesh))
    if args.json:
        res = {"splats": os.path.abspath(args.splats), "dataset": os.path.abspath(args.dataset),
               "grid": {"dims": list(dims), "voxel_size": voxel, "origin": list(origin), "trunc": vol.trunc,
                        "bytes": vol.nbytes},
               "views": args.views, "num_views": len(views), "antialiased": bool(args.antialiased),
               "use_masks": not args.no_masks, "alpha_min": args.alpha_min, "max_depth": args.max_depth,
               "min_views": args.min_views, "depth": args.depth, "median_level": args.median_level,
               "observed_fraction": observed, "vertices": nv, "faces": nf}
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
