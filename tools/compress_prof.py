#!/usr/bin/env python3
"""Cost of the compressed splat export and import on one synthetic cloud (default S1: 1 048 576 splats, SH degree 3),
alternating call by call in one process after a warm-up, device events, median and spread of `iters` rounds:
  * pack: brush_splat_pack_keys + the 30-bit stable argsort + brush_splat_pack (pack_splats), and its three parts;
    brush_splat_pack once more with the identity as the order, which takes the gather out of the same kernel (the
    synthetic cloud is in random order, so its Morton order is a random permutation: the worst case of the gather);
  * unpack: brush_splat_unpack (PackedSplats.unpack's kernel alone, outputs allocated once);
  * the achieved bytes per second over the bytes each part MUST move (pack: 236 B read + 61 B written per splat at
    degree 3; keys: 236 B read + 8 B written; unpack: 61 B read + 236 B written), computed from the shapes;
  * beside them the full-width device-to-host copy of the five parameter tensors that Splats.to_ply makes today and
    the copy of the packed arrays that PackedSplats.to_ply makes, host clock around a synchronised copy.
Meant to run under `rocprofv3 --kernel-trace --stats` as well, in a run of its own, for k_pack_bounds / k_pack_keys /
k_splat_pack / k_splat_unpack next to the sort's kernels.

    python tools/compress_prof.py [--splats 1048576] [--sh-degree 3] [--iters 20] [--json F]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/compress_prof.py --iters 10

profiles/compress_prof.json is the first form's output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import brush_amd  # noqa: E402
from brush_amd import _lib  # noqa: E402
from brush_amd import compress as Cm  # noqa: E402
from brush_amd.synthetic import synthetic_cloud  # noqa: E402


def _timed(fns, iters):
    """{name: (median ms, min ms, max ms)} of device-event times for the callables of `fns`, called in alternation."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def _host_timed(fn, iters):
    """(median, min, max) ms of a host clock around fn() between two device synchronisations."""
    ts = []
    for i in range(iters + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=1 << 20)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, deg = a.splats, a.sh_degree
    c = synthetic_cloud(n, deg, seed=4)
    splats = brush_amd.Splats(*(torch.from_numpy(c[k]).to(dev) for k in ("means", "sh", "quats", "raw_opac",
                                                                         "log_scales")))
    params, _ = Cm._device_params(splats)
    coeffs = (deg + 1) ** 2
    rest = 3 * (coeffs - 1)
    raw_b, packed_b = 4 * (14 + rest), 16 + rest  # per splat (the 72 B per chunk are 0.28 B per splat more)
    l = _lib.lib()
    stream = _lib.current_stream(dev)

    packed = Cm.pack_splats(splats)
    order = packed.order
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    keys, vals, keys_out, order_out, state = i32(n), i32(n), i32(n), i32(n), i32(2)
    ws_b = _lib.size_query("brush_splat_pack_workspace_size", n)
    sort_b = _lib.size_query("brush_radix_argsort_workspace_size", n)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    sort_ws = torch.empty(max(sort_b, 1), dtype=torch.uint8, device=dev)
    chunks_n = -(-n // 256)
    chunks = torch.empty((chunks_n, 18), dtype=torch.float32, device=dev)
    words = i32(chunks_n * 256, 4)
    sh = torch.empty((chunks_n * 256, rest), dtype=torch.uint8, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    o_means, o_scales, o_rot, o_opac, o_sh = f32(n, 3), f32(n, 3), f32(n, 4), f32(n), f32(n, coeffs, 3)
    ptrs = [p.data_ptr() for p in params]

    def run_keys():
        _lib.check(l.brush_splat_pack_keys(*ptrs, n, deg, keys.data_ptr(), vals.data_ptr(), state.data_ptr(),
                                           ws.data_ptr(), ws_b, stream), "brush_splat_pack_keys")

    def run_sort():
        _lib.check(l.brush_radix_argsort_u32(keys.data_ptr(), vals.data_ptr(), keys_out.data_ptr(),
                                             order_out.data_ptr(), state.data_ptr(), n, 30, sort_ws.data_ptr(), sort_b,
                                             stream), "brush_radix_argsort_u32")

    def run_pack():
        _lib.check(l.brush_splat_pack(*ptrs, n, deg, deg, order.data_ptr(), chunks.data_ptr(), words.data_ptr(),
                                      sh.data_ptr() if rest else None, stream), "brush_splat_pack")

    identity = torch.arange(n, dtype=torch.int32, device=dev)

    def run_pack_identity():  # the same kernel without the gather: rows in index order (other words, same traffic)
        _lib.check(l.brush_splat_pack(*ptrs, n, deg, deg, identity.data_ptr(), chunks.data_ptr(), words.data_ptr(),
                                      sh.data_ptr() if rest else None, stream), "brush_splat_pack")

    def run_unpack():
        _lib.check(l.brush_splat_unpack(packed.chunks.data_ptr(), packed.words.data_ptr(),
                                        packed.sh.data_ptr() if rest else None, n, deg, o_means.data_ptr(),
                                        o_scales.data_ptr(), o_rot.data_ptr(), o_opac.data_ptr(), o_sh.data_ptr(),
                                        stream), "brush_splat_unpack")

    # a device copy moving the pack's byte counts (a copy of B bytes reads B and writes B), as a yardstick
    src = torch.empty((raw_b + packed_b) * n // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    run_keys()
    fns = {"pack_splats_ms": lambda: Cm.pack_splats(splats), "keys_ms": run_keys, "sort_ms": run_sort,
           "pack_ms": run_pack, "pack_index_order_ms": run_pack_identity, "unpack_ms": run_unpack,
           "copy_same_bytes_ms": lambda: dst.copy_(src)}
    t = _timed(fns, a.iters)
    moved = {"keys_ms": raw_b + 8, "pack_ms": raw_b + packed_b + 4, "pack_index_order_ms": raw_b + packed_b + 4,
             "unpack_ms": raw_b + packed_b, "copy_same_bytes_ms": raw_b + packed_b}
    res = {}
    for k, (med, lo, hi) in t.items():
        res[k] = {"median": med, "min": lo, "max": hi}
        if k in moved:
            res[k]["bytes_per_splat"] = moved[k]
            res[k]["gb_per_s"] = moved[k] * n / (med * 1e-3) / 1e9
    tensors = [getattr(splats, k).detach() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")]
    full = _host_timed(lambda: [p.cpu() for p in tensors], max(3, a.iters // 4))
    small = _host_timed(lambda: torch.cat([x.contiguous().view(torch.uint8).reshape(-1)
                                           for x in (packed.chunks, packed.words, packed.sh)]).cpu(),
                        max(3, a.iters // 4))
    res["to_ply_full_width_d2h_ms"] = {"median": full[0], "min": full[1], "max": full[2], "bytes": raw_b * n}
    res["packed_d2h_ms"] = {"median": small[0], "min": small[1], "max": small[2], "bytes": packed.nbytes}
    line = {"splats": n, "sh_degree": deg, "iters": a.iters, "device": torch.cuda.get_device_name(dev),
            "bytes_per_splat_raw": raw_b, "bytes_per_splat_packed": packed_b, **res}
    print(json.dumps(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
