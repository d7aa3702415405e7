"""Prune a splat file by rendered contribution (brush_amd/contribution.py).

    python -m brush_amd.prune SPLATS DATASET [--min-contribution 0.01 | --keep-fraction F [--by max|sum]]
                              [--views train|eval|all] [--antialiased] [--export OUT.ply] [--json OUT.json]
                              [--format auto|nerf|colmap] [--eval-split-every K] [--max-resolution R] [--no-undistort]

Measures every splat's contribution over the chosen views (default: the training views), drops the splats whose
largest blending weight stays below --min-contribution (RadSplat's rule; 0 drops only splats that are never composited
and never stop a pixel, which changes no bit of those views) or keeps the --keep-fraction largest by max or summed
weight (LightGaussian's ranking), and prints the splat count and, when the dataset has eval views, their mean PSNR and
SSIM (eval_stats) before and after.  --json holds the same numbers plus the histogram of `max` in decades.
"""
from __future__ import annotations

from . import cli


def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.prune",
                                description="prune splats by their rendered contribution to a dataset's views")
    p.add_argument("splats", help=".ply or .safetensors splat file")
    p.add_argument("dataset", help="dataset directory or .zip (NeRF-synthetic or COLMAP)")
    p.add_argument("--min-contribution", type=float, default=None, metavar="T",
                   help="prune splats whose largest blending weight over the views is below T (default 0.01; 0: only "
                        "splats that are never composited and never stop a pixel)")
    p.add_argument("--keep-fraction", type=float, default=None, metavar="F",
                   help="instead: keep the ceil(F N) splats that rank highest by --by")
    p.add_argument("--by", choices=("max", "sum"), default="max", help="--keep-fraction: the ranking key")
    cli.add_views_option(p, "train", "the views the contribution is measured over")
    cli.add_antialiased_option(p)
    cli.add_export_option(p, "the kept splats", metavar="OUT.ply")
    cli.add_json_option(p, metavar="OUT.json")
    cli.add_dataset_options(p)
    return p


def rule_from_args(args) -> dict:
    """The keyword arguments of prune_mask the command line asks for; ValueError when both rules are given or a value
    is out of range."""
    if args.min_contribution is not None and args.keep_fraction is not None:
        raise ValueError("--min-contribution and --keep-fraction are two rules: give one of them")
    if args.keep_fraction is not None:
        if not 0.0 <= args.keep_fraction <= 1.0:
            raise ValueError(f"--keep-fraction must be in [0, 1], got {args.keep_fraction}")
        return {"keep_fraction": float(args.keep_fraction), "by": args.by}
    t = 0.01 if args.min_contribution is None else float(args.min_contribution)
    if not 0.0 <= t <= 1.0:
        raise ValueError(f"--min-contribution must be in [0, 1], got {t}")
    return {"min_max": t}


def main(argv=None) -> int:
    import os

    p = parser()
    args = p.parse_args(argv)
    try:
        rule = rule_from_args(args)
    except ValueError as e:
        p.error(str(e))
    got = cli.dataset_views(args, args.views)  # host work and the refusals first
    if got is None:
        return 2
    from .contribution import max_histogram, prune_mask, splat_contributions
    from .eval import eval_stats

    data, views, dev = got
    has_eval = bool(cli.chosen_views(data, "eval"))
    splats = cli.load_splats(args.splats, dev)

    def score(s):
        if not has_eval:
            return None
        st = eval_stats(s, data.eval, antialiased=args.antialiased)
        return {"psnr": st.mean_psnr(), "ssim": st.mean_ssim(), "views": len(st.samples)}

    c = splat_contributions(splats, views, antialiased=args.antialiased)
    mask = prune_mask(c, **rule)
    kept = splats.select((~mask).to(dev))
    before, after = score(splats), score(kept)
    n0, n1 = splats.num_splats(), kept.num_splats()
    print(f"splats\tbefore {n0}\tafter {n1}\t({len(views)} {args.views} views)")
    if has_eval:
        print(f"eval ({before['views']} views)\tpsnr {before['psnr']:.4f} -> {after['psnr']:.4f}\t"
              f"ssim {before['ssim']:.6f} -> {after['ssim']:.6f}")
    if args.export:
        cli.export_splats(args.export, kept)
    if args.json:
        res = {"splats": os.path.abspath(args.splats), "dataset": os.path.abspath(args.dataset), "rule": rule,
               "views": args.views, "num_views": len(views), "antialiased": bool(args.antialiased),
               "splats_before": n0, "splats_after": n1, "eval_before": before, "eval_after": after,
               "max_histogram": max_histogram(c)}
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
