"""What the command lines share (eval, train_loop, prune, lift, mesh, compress): the option rows every one of them
declares, and the steps between parsing and the work itself: read the dataset on the host, choose its views, refuse an
empty choice with status 2 before any device work, pick the device, undistort, load the splats; and afterwards write
--export and --json.  torch is imported where a step needs it, so that a parser costs no more than argparse.
"""
from __future__ import annotations

import sys


def add_dataset_options(p):
    """--format, --eval-split-every, --max-resolution: what read_args_dataset reads; --no-undistort."""
    p.add_argument("--format", choices=("auto", "nerf", "colmap"), default="auto")
    p.add_argument("--eval-split-every", type=int, default=None)
    p.add_argument("--max-resolution", type=int, default=None)
    p.add_argument("--no-undistort", action="store_true",
                   help="use views with lens distortion (COLMAP SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV) as loaded, "
                        "as if they were pinhole, instead of undistorting them first")


def add_views_option(p, default: str, help: str):
    p.add_argument("--views", choices=("train", "eval", "all"), default=default, help=help)


def add_antialiased_option(p, help: str = "render in the antialiased mode (opacity compensation of the 2D blur), e.g. "
                                          "for splats trained with it"):
    p.add_argument("--antialiased", action="store_true", help=help)


def add_json_option(p, metavar=None, help: str = "also write the results to this file"):
    p.add_argument("--json", default=None, metavar=metavar, help=help)


def add_export_option(p, what: str, metavar=None):
    """--export for a command that writes splats (export_splats); `what`: the splats it writes."""
    p.add_argument("--export", default=None, metavar=metavar,
                   help=f"write {what} to this .ply (a name ending in .compressed.ply: the chunk-quantised layout, "
                        "brush_amd/compress.py)")


def read_args_dataset(args):
    """The Dataset the options of add_dataset_options name; host only."""
    from .dataset import read_dataset

    return read_dataset(args.dataset, args.format, max_resolution=args.max_resolution,
                        eval_split_every=args.eval_split_every)


def chosen_views(data, which: str) -> list:
    """The views --views names: 'train', 'eval' (empty when the dataset has none) or 'all', training views first."""
    ev = list(data.eval.views) if data.eval is not None else []
    return {"train": list(data.train.views), "eval": ev, "all": list(data.train.views) + ev}[which]


def no_views(args, which: str) -> int:
    """The refusal of an empty choice: one line on stderr; returns the exit status."""
    print(f"{args.dataset}: the dataset has no {which} views", file=sys.stderr)
    return 2


def cuda_device():
    import torch

    return torch.device("cuda", torch.cuda.current_device())


def dataset_views(args, which: str):
    """(dataset, the `which` views of it, device) for a command that works on views of args.dataset: read on the host,
    an empty choice refused (no_views) with None as the result before any device work, then undistorted on the device
    unless --no-undistort, the views chosen again since distorted views have become pinhole views."""
    from .undistort import undistort_for_cli

    data = read_args_dataset(args)
    if not chosen_views(data, which):
        no_views(args, which)
        return None
    dev = cuda_device()
    data = undistort_for_cli(data, not args.no_undistort, dev)
    return data, chosen_views(data, which), dev


def load_splats(path: str, dev):
    """Splats of a .safetensors file, else of a PLY (float or compressed)."""
    from .gaussian_splats import Splats

    return (Splats.from_safetensors if path.endswith(".safetensors") else Splats.from_ply)(path, dev)


def export_splats(path: str, splats):
    from .compress import ply_bytes_for  # OUT.compressed.ply: the compressed layout

    with open(path, "wb") as f:
        f.write(ply_bytes_for(splats, path))


def write_json(path: str, obj):
    import json

    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
