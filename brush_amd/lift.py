"""Lift 2D label images onto the splats of a trained scene (brush_amd/features.py; FlashSplat's closed-form label
transfer is the model), and cut an object out.

    python -m brush_amd.lift SPLATS DATASET --labels DIR [--num-classes K] [--views train|eval|all] [--antialiased]
                             [--no-undistort] [--min-weight W] [--export-labels OUT.npy]
                             [--select CLASS --export OUT.ply] [--render-dir DIR] [--json OUT.json]
                             [--format auto|nerf|colmap] [--eval-split-every K] [--max-resolution R]

DIR holds one 8-bit single-channel (grey or palette) PNG per view, DIR/<image name>.png or DIR/<stem>.png, looked up as
masks/ are; a pixel's value is its class id, 255 (or anything >= K) is "unlabelled".  A label image of another size than
the view is resized to it by nearest neighbour, and with lens distortion it is remapped with the view, as a loss mask
is (pixels without a source become unlabelled); pixels a loss mask rules out are unlabelled too.  Every splat takes the
class whose pixels it contributed the most blending weight to, -1 where no class received more than --min-weight (in
pixels of full weight).  The geometry is frozen: no parameter changes.

--export-labels writes the int32 [N] labels; --select CLASS --export OUT.ply writes the splats of that class
(Splats.select); --render-dir writes, per eval view, the argmax of the rendered one-hot class features as an 8-bit PNG,
255 where all channels are zero: the visual check of the lift; --json holds the per-class splat counts and weights.
"""
from __future__ import annotations

import os

from . import cli

IGNORE = 255


def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.lift",
                                description="lift per-view label images onto the splats of a scene")
    p.add_argument("splats", help=".ply or .safetensors splat file")
    p.add_argument("dataset", help="dataset directory or .zip (NeRF-synthetic or COLMAP)")
    p.add_argument("--labels", required=True, metavar="DIR", help="directory of 8-bit single-channel label PNGs")
    p.add_argument("--num-classes", type=int, default=None, metavar="K",
                   help="class ids are 0..K-1 (default: the largest id found below 255, plus one); at most 64")
    cli.add_views_option(p, "train", "the views that vote")
    cli.add_antialiased_option(p)
    p.add_argument("--min-weight", type=float, default=0.0, metavar="W",
                   help="a splat whose best class received no more than W pixels of full weight stays unlabelled (-1)")
    p.add_argument("--export-labels", default=None, metavar="OUT.npy", help="write the int32 [N] labels")
    p.add_argument("--select", type=int, default=None, metavar="CLASS", help="with --export: the class to cut out")
    cli.add_export_option(p, "the splats of --select", metavar="OUT.ply")
    p.add_argument("--render-dir", default=None, metavar="DIR",
                   help="write the rendered label image of every eval view here")
    cli.add_json_option(p, metavar="OUT.json")
    cli.add_dataset_options(p)
    return p


def check_args(args):
    """ValueError for combinations the command line cannot serve."""
    if (args.select is None) != (args.export is None):
        raise ValueError("--select CLASS and --export OUT.ply go together")
    if args.num_classes is not None and not 1 <= args.num_classes <= 64:
        raise ValueError(f"--num-classes must be in [1, 64], got {args.num_classes}: remap the labels")
    if args.select is not None and args.select < 0:
        raise ValueError(f"--select must be a class id >= 0, got {args.select}")
    if not args.min_weight >= 0.0:
        raise ValueError(f"--min-weight must be >= 0, got {args.min_weight}")


def find_label_file(labels_dir: str, view_name: str):
    """The label image of the view whose image is <...>/<name>: DIR/<name>.png, else DIR/<stem>.png (the lookup of
    masks/), or None."""
    name = os.path.basename(view_name.replace("\\", "/"))
    stem = os.path.splitext(name)[0]
    for cand in (f"{name}.png", f"{stem}.png"):
        path = os.path.join(labels_dir, cand)
        if os.path.isfile(path):
            return path
    return None


def decode_labels(path: str):
    """A label PNG as uint8 [h,w]: 8-bit grey ("L") or palette ("P": the indices are the class ids); anything else is a
    ValueError naming the file."""
    import numpy as np
    from PIL import Image

    img = Image.open(path)
    if img.mode not in ("L", "P"):
        raise ValueError(f"{path}: a label image must be 8-bit single channel (grey or palette), got mode {img.mode}")
    return np.ascontiguousarray(np.asarray(img), dtype=np.uint8)


def with_labels_as_masks(views, labels_dir: str):
    """Copies of `views` whose `mask` field carries the label image SHIFTED by one modulo 256 (unlabelled 255 -> 0, class
    k -> k + 1), at the view's size, so that whatever a loss mask goes through (the undistortion's nearest remap, where
    a pixel without a source becomes 0) treats the labels correctly; labels_of() undoes the shift.  Pixels the view's
    own loss mask rules out are unlabelled.  A view without a label file is a ValueError."""
    import dataclasses

    import numpy as np

    from .dataset import resize_nearest

    out = []
    for v in views:
        path = find_label_file(labels_dir, v.name)
        if path is None:
            raise ValueError(f"{v.name}: no label image {os.path.basename(v.name)}.png or <stem>.png in {labels_dir}")
        lab = decode_labels(path)
        hw = tuple(v.image.shape[:2])
        if tuple(lab.shape) != hw:
            lab = resize_nearest(lab, hw)
        if getattr(v, "mask", None) is not None:
            lab = np.where(v.mask != 0, lab, np.uint8(IGNORE)).astype(np.uint8)
        out.append(dataclasses.replace(v, mask=(lab.astype(np.int32) + 1).astype(np.uint8)))  # 255 + 1 wraps to 0
    return out


def labels_of(view):
    """The uint8 [h,w] label image a view of with_labels_as_masks carries."""
    import numpy as np

    return np.ascontiguousarray((view.mask.astype(np.int32) - 1).astype(np.uint8))  # 0 - 1 wraps to 255


def main(argv=None) -> int:
    import sys

    p = parser()
    args = p.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        p.error(str(e))
    import numpy as np
    import torch

    from .dataset import Dataset
    from .features import lift_labels
    from .undistort import undistort_for_cli

    data = cli.read_args_dataset(args)  # before any GPU work
    has_eval = bool(cli.chosen_views(data, "eval"))
    try:
        voting = with_labels_as_masks(cli.chosen_views(data, args.views), args.labels)
    except ValueError as e:
        print(str(e), file=sys.stderr)
        return 2
    if not voting:
        return cli.no_views(args, args.views)
    dev = cli.cuda_device()
    # the voting views, labels in the mask field, through the same undistortion as every command line applies
    voting = undistort_for_cli(Dataset.from_views(voting, []), not args.no_undistort, dev).train.views
    label_maps = [labels_of(v) for v in voting]
    k = args.num_classes
    if k is None:
        k = 1 + max((int(m[m != IGNORE].max()) for m in label_maps if (m != IGNORE).any()), default=0)
        if k > 64:
            print(f"the label images hold class ids up to {k - 1}: at most 64 classes, remap them", file=sys.stderr)
            return 2
    splats = cli.load_splats(args.splats, dev)
    labels, sums = lift_labels(splats, voting, label_maps, k, min_weight=args.min_weight, antialiased=args.antialiased,
                               use_masks=False)  # (the loss masks are already in the labels)
    got = labels.cpu().numpy()
    r = sums.read()
    weights = (r.sum.to(torch.float64) / float(1 << 24)).sum(dim=0).tolist()
    counts = [int((got == c).sum()) for c in range(k)]
    print(f"splats {splats.num_splats()}\tlabelled {int((got >= 0).sum())}\tunlabelled {int((got < 0).sum())}\t"
          f"({len(voting)} {args.views} views, {k} classes)")
    for c in range(k):
        print(f"class {c}\tsplats {counts[c]}\tweight {weights[c]:.1f}")
    if args.export_labels:
        np.save(args.export_labels, got.astype(np.int32))
    if args.export:
        cli.export_splats(args.export, splats.select(labels == args.select))
    rendered = 0
    if args.render_dir and has_eval:
        from PIL import Image

        os.makedirs(args.render_dir, exist_ok=True)
        hot = torch.nn.functional.one_hot(labels.clamp_min(0).long(), k).to(torch.float32)
        hot = torch.where((labels >= 0).unsqueeze(1), hot, torch.zeros_like(hot)).contiguous()
        for v in undistort_for_cli(data, not args.no_undistort, dev).eval.views:
            h, w = v.image.shape[:2]
            with torch.no_grad():
                _, feat, _ = splats.render_features(v.camera, (w, h), hot, antialiased=args.antialiased)
            arg = torch.where(feat.amax(dim=2) > 0, feat.argmax(dim=2), torch.full((h, w), IGNORE, device=dev))
            stem = os.path.splitext(os.path.basename(v.name.replace("\\", "/")))[0]
            Image.fromarray(arg.to(torch.uint8).cpu().numpy(), mode="L").save(os.path.join(args.render_dir,
                                                                                          f"{stem}.png"))
            rendered += 1
    if args.json:
        res = {"splats": os.path.abspath(args.splats), "dataset": os.path.abspath(args.dataset),
               "labels": os.path.abspath(args.labels), "views": args.views, "num_views": len(voting),
               "antialiased": bool(args.antialiased), "num_classes": k, "min_weight": float(args.min_weight),
               "num_splats": splats.num_splats(), "unlabelled": int((got < 0).sum()),
               "classes": [{"class": c, "splats": counts[c], "weight": weights[c]} for c in range(k)],
               "rendered_views": rendered}
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
