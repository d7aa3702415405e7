"""Compressed splat export and import: the chunk-quantised PLY layout, packed and unpacked on the device.

    python -m brush_amd.compress SPLATS [--sh-degree D] [--export OUT.compressed.ply]
                                 [--dataset DIR [--views train|eval|all] [--antialiased]] [--json OUT.json]
                                 [--format auto|nerf|colmap] [--eval-split-every K] [--max-resolution R]

The layout other trainers and viewers exchange as "compressed PLY": the splats sorted along a Morton curve, chunks of 256
rows with the min and max of position, scale and colour, four 32-bit words per splat and one byte per higher-order SH
value: 16 B + 3K B per splat (61 B at SH degree 3, 16 B at degree 0) against 236 B in the float file.
include/brush_hip.h states every word; brush_amd/csrc/splat_pack.hip holds the three kernels.

`pack_splats` runs on the parameters where they are: brush_splat_pack_keys, the library's stable radix argsort and
brush_splat_pack, launches only; `PackedSplats.to_ply` then reads 61 B per splat back instead of 236.
`PackedSplats.from_ply(...).unpack()` uploads the packed arrays and runs brush_splat_unpack.  `Splats.from_ply` /
`Splats.to_compressed_ply` and every `--export OUT.compressed.ply` go through here.

The command line prints the raw and compressed byte counts and the largest absolute round-trip error per parameter
group; with a dataset it renders the chosen views from the original and from the round-tripped splats (eval_stats) and
prints PSNR / SSIM of both against the ground truth and the PSNR of one render against the other.  Reported, not gated.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, cli
from .ply import CHUNK, compressed_to_ply, load_compressed_ply, sh_rest_count

_DEGREE_OF_COEFFS = {1: 0, 4: 1, 9: 2, 16: 3}
COMPRESSED_SUFFIX = ".compressed.ply"


def _degree_of(sh_coeffs: torch.Tensor) -> int:
    if sh_coeffs.dim() != 3 or sh_coeffs.shape[2] != 3 or int(sh_coeffs.shape[1]) not in _DEGREE_OF_COEFFS:
        raise ValueError(f"the compressed layout holds SH degrees 0 to 3 (sh_coeffs [N, 1 | 4 | 9 | 16, 3]), got "
                         f"{tuple(sh_coeffs.shape)}")
    return _DEGREE_OF_COEFFS[int(sh_coeffs.shape[1])]


def _device_params(splats):
    """The five parameters as the kernels read them (detached, contiguous float32 device tensors), after sync()."""
    splats.sync()
    params = [getattr(splats, k).detach() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")]
    if not all(p.is_cuda for p in params):
        raise ValueError("the packer runs on the device: the splats' tensors must live on the GPU")
    n = int(params[0].shape[0])
    if n == 0:
        raise ValueError("No splats to pack")
    params = [p.contiguous().float() for p in params]
    # rotation and SH rows are read as whole 16-byte words: a view that starts inside an allocation is copied
    return [p.clone() if p.data_ptr() % 16 else p for p in params], n


def _keys_and_order(params, n: int, sh_degree: int, stream):
    """(order int32 [n], state int32 [2]): brush_splat_pack_keys and the stable argsort of its keys, launches only."""
    dev = params[0].device
    l = _lib.lib()
    keys, vals, keys_out, order = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    state = torch.empty(2, dtype=torch.int32, device=dev)
    ws_bytes = _lib.size_query("brush_splat_pack_workspace_size", n)
    sort_bytes = _lib.size_query("brush_radix_argsort_workspace_size", n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    sort_ws = torch.empty(max(sort_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(l.brush_splat_pack_keys(*(p.data_ptr() for p in params), n, sh_degree, keys.data_ptr(), vals.data_ptr(),
                                       state.data_ptr(), ws.data_ptr(), ws_bytes, stream), "brush_splat_pack_keys")
    _lib.check(l.brush_radix_argsort_u32(keys.data_ptr(), vals.data_ptr(), keys_out.data_ptr(), order.data_ptr(),
                                         state.data_ptr(), n, 30, sort_ws.data_ptr(), sort_bytes, stream),
               "brush_radix_argsort_u32")
    return order, state


def morton_order(means: torch.Tensor) -> torch.Tensor:
    """The packed order of a cloud: int32 [N] on the means' device, the splat indices stably sorted by the 30-bit
    Morton code of the means quantised to 1024 cells per axis of their bounding box (ties keep index order)."""
    if not isinstance(means, torch.Tensor) or not means.is_cuda:
        raise ValueError("the packer runs on the device: means must be a GPU tensor")
    if means.dim() != 2 or means.shape[1] != 3 or means.shape[0] == 0:
        raise ValueError(f"means must be [N,3] with N > 0, got {tuple(means.shape)}")
    means = means.detach().contiguous().float()
    n = int(means.shape[0])
    # the entry reads every parameter for its non-finite flag: the other four are zeros of their own sizes
    dev = means.device
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    params = [means, zeros(n, 3), zeros(n, 4), zeros(n), zeros(n, 1, 3)]
    with torch.cuda.device(dev):
        return _keys_and_order(params, n, 0, _lib.current_stream())[0]


@dataclass
class PackedSplats:
    """A cloud in the compressed layout, on a device.  `order` is None for a cloud read from a file."""
    chunks: torch.Tensor            # float32 [C,18], C = ceil(N / 256)
    words: torch.Tensor             # int32 [N,4]: position, rotation, scale, colour + opacity
    sh: torch.Tensor                # uint8 [N,3K]
    order: Optional[torch.Tensor]   # int32 [N]: row i is input splat order[i]
    sh_degree: int
    nonfinite: Optional[torch.Tensor] = None  # int32 [1] on the device: 1 when a parameter was an infinity or a NaN

    @property
    def num_splats(self) -> int:
        return int(self.words.shape[0])

    @property
    def nbytes(self) -> int:
        """Bytes of the packed arrays (the file's body): 72 per chunk, 16 + 3K per splat."""
        return sum(int(t.numel()) * t.element_size() for t in (self.chunks, self.words, self.sh))

    def to_ply(self) -> bytes:
        """The compressed PLY.  One read-back: the flag and the three arrays leave the device as one byte buffer.
        ValueError when a parameter of the packed cloud was not finite."""
        as_bytes = lambda t: t.contiguous().view(torch.uint8).reshape(-1)
        flag = self.nonfinite if self.nonfinite is not None else torch.zeros(1, dtype=torch.int32,
                                                                            device=self.words.device)
        host = torch.cat([as_bytes(flag), as_bytes(self.chunks), as_bytes(self.words), as_bytes(self.sh)]).cpu().numpy()
        if host[:4].view(np.int32)[0] != 0:
            raise ValueError("the splats hold a non-finite parameter (an infinity or a NaN): nothing was written")
        n, c = self.num_splats, int(self.chunks.shape[0])
        a, b = 4 + c * 72, 4 + c * 72 + n * 16
        return compressed_to_ply(host[4:a].view(np.float32).reshape(c, 18), host[a:b].view(np.uint32).reshape(n, 4),
                                 host[b:].reshape(n, int(self.sh.shape[1])))

    @classmethod
    def from_ply(cls, path_or_bytes, device) -> "PackedSplats":
        """Uploads the packed arrays of a compressed PLY (ply.load_compressed_ply) as they are."""
        chunks, words, sh = load_compressed_ply(path_or_bytes)
        degree = {0: 0, 9: 1, 24: 2, 45: 3}[sh.shape[1]]
        up = lambda a: torch.from_numpy(a).to(device)
        return cls(up(chunks), up(words.view(np.int32)), up(sh), None, degree)

    def unpack(self):
        """The cloud as Splats on this one's device, rows in packed order (brush_splat_unpack).  The rotations are
        what the file holds, of unit length to the quantisation step; Splats.from_ply normalises them afterwards."""
        from .gaussian_splats import Splats

        dev = self.words.device
        if not self.words.is_cuda:
            raise ValueError("the unpacker runs on the device: the packed arrays must live on the GPU")
        n, coeffs = self.num_splats, sh_rest_count(self.sh_degree) + 1
        chunks, words, sh = self.chunks.contiguous(), self.words.contiguous(), self.sh.contiguous()
        if tuple(chunks.shape) != (-(-n // CHUNK), 18) or tuple(sh.shape) != (n, 3 * (coeffs - 1)):
            raise ValueError(f"{n} packed splats of SH degree {self.sh_degree} need chunks {(-(-n // CHUNK), 18)} and "
                             f"sh {(n, 3 * (coeffs - 1))}, got {tuple(chunks.shape)} and {tuple(sh.shape)}")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        means, log_scales, rotation, raw_opacity, sh_coeffs = new(n, 3), new(n, 3), new(n, 4), new(n), new(n, coeffs, 3)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().brush_splat_unpack(chunks.data_ptr(), words.data_ptr(),
                                                     sh.data_ptr() if coeffs > 1 else None, n, self.sh_degree,
                                                     means.data_ptr(), log_scales.data_ptr(), rotation.data_ptr(),
                                                     raw_opacity.data_ptr(), sh_coeffs.data_ptr(),
                                                     _lib.current_stream()), "brush_splat_unpack")
        return Splats(means, sh_coeffs, rotation, raw_opacity, log_scales)


def pack_splats(splats, *, sh_degree: Optional[int] = None) -> PackedSplats:
    """The splats in the compressed layout, on their device: pending SH optimizer steps are applied (Splats.sync), then
    keys, sort and pack are enqueued on the current stream; nothing is read back or synchronised.  `sh_degree`: the
    degree written (None: the splats'); a lower one drops the bands above it, a higher one is a ValueError."""
    params, n = _device_params(splats)
    degree_in = _degree_of(params[4])
    degree = degree_in if sh_degree is None else int(sh_degree)
    if not 0 <= degree <= degree_in:
        raise ValueError(f"sh_degree must be in [0, {degree_in}] (the splats' degree), got {sh_degree}")
    dev = params[0].device
    num_chunks, rest = -(-n // CHUNK), sh_rest_count(degree)
    # whole chunks: the kernel writes the rows behind n (as zeros) and a chunk's SH bytes as whole 32-bit words
    chunks = torch.empty((num_chunks, 18), dtype=torch.float32, device=dev)
    words = torch.empty((num_chunks * CHUNK, 4), dtype=torch.int32, device=dev)
    sh = torch.empty((num_chunks * CHUNK, 3 * rest), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.current_stream()
        order, state = _keys_and_order(params, n, degree_in, stream)
        _lib.check(_lib.lib().brush_splat_pack(*(p.data_ptr() for p in params), n, degree_in, degree, order.data_ptr(),
                                               chunks.data_ptr(), words.data_ptr(), sh.data_ptr() if rest else None,
                                               stream), "brush_splat_pack")
    return PackedSplats(chunks, words[:n], sh[:n], order, degree, state[1:2])


def ply_bytes_for(splats, path: str) -> bytes:
    """What an `--export PATH` writes: the compressed PLY when the name ends in .compressed.ply, else the float PLY."""
    if str(path).endswith(COMPRESSED_SUFFIX):
        return splats.to_compressed_ply()
    return splats.to_ply()


# ---------------------------------------------------------------------------- command line
def parser():
    import argparse

    p = argparse.ArgumentParser(prog="python -m brush_amd.compress",
                                description="pack a splat file into the compressed PLY layout and report what it costs")
    p.add_argument("splats", help=".ply (float or compressed) or .safetensors splat file")
    p.add_argument("--sh-degree", type=int, default=None, metavar="D", help="write SH bands up to D (default: all)")
    p.add_argument("--export", default=None, metavar="OUT.compressed.ply", help="write the compressed PLY here")
    p.add_argument("--dataset", default=None, metavar="DIR",
                   help="dataset directory or .zip: render its views from the original and the round-tripped splats")
    cli.add_views_option(p, "eval", "with --dataset: the views rendered")
    cli.add_antialiased_option(p)
    cli.add_json_option(p, metavar="OUT.json")
    cli.add_dataset_options(p)
    return p


def raw_nbytes(n: int, sh_coeffs: int) -> int:
    """Bytes of the float PLY's body: 14 + 3 (coefficients - 1) floats per splat."""
    return n * 4 * (14 + 3 * (sh_coeffs - 1))


@torch.no_grad()
def roundtrip_errors(splats, packed: PackedSplats, back) -> dict:
    """Largest absolute difference per parameter group between the splats (in packed order, SH bands cut to the packed
    degree, rotations normalised and sign-aligned) and their round trip `back`; device work and one read-back."""
    order = packed.order.long()
    coeffs = back.sh_coeffs.shape[1]
    rot = splats.rotation.detach()[order]
    rot = rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))
    rot_back = back.rotation.detach()
    sign = torch.where(torch.sum(rot * rot_back, dim=1, keepdim=True) < 0, -1.0, 1.0)
    alpha = lambda t: torch.sigmoid(t.detach())
    diffs = {
        "means": splats.means.detach()[order] - back.means.detach(),
        "log_scales": splats.log_scales.detach()[order].clamp(-20.0, 20.0) - back.log_scales.detach(),
        "rotation": rot * sign - rot_back,
        "opacity": alpha(splats.raw_opacity)[order] - alpha(back.raw_opacity),
        "sh_dc": splats.sh_coeffs.detach()[order][:, 0] - back.sh_coeffs.detach()[:, 0],
    }
    if coeffs > 1:
        diffs["sh_rest"] = splats.sh_coeffs.detach()[order][:, 1:coeffs] - back.sh_coeffs.detach()[:, 1:]
    host = torch.stack([d.abs().max() for d in diffs.values()]).cpu().tolist()
    return dict(zip(diffs, (float(v) for v in host)))


def main(argv=None) -> int:
    import os

    args = parser().parse_args(argv)
    data = cli.read_args_dataset(args) if args.dataset else None  # before any GPU work
    dev = cli.cuda_device()
    splats = cli.load_splats(args.splats, dev)
    packed = pack_splats(splats, sh_degree=args.sh_degree)
    blob = packed.to_ply()  # raises for non-finite parameters
    back = PackedSplats.from_ply(blob, dev).unpack()
    back.norm_rotations()
    n = splats.num_splats()
    res = {"splats": os.path.abspath(args.splats), "num_splats": n, "sh_degree": packed.sh_degree,
           "bytes_raw": raw_nbytes(n, int(splats.sh_coeffs.shape[1])), "bytes_compressed": packed.nbytes,
           "file_bytes_compressed": len(blob), "max_abs_error": roundtrip_errors(splats, packed, back)}
    print(f"splats\t{n}\tSH degree {packed.sh_degree}")
    print(f"bytes\traw {res['bytes_raw']}\tcompressed {res['bytes_compressed']}\t"
          f"({res['bytes_compressed'] / res['bytes_raw']:.4f} of raw)")
    print("max |round trip - original|\t" + "\t".join(f"{k} {v:.3e}" for k, v in res["max_abs_error"].items()))
    if data is not None:
        from .dataset import Scene
        from .eval import eval_stats
        from .undistort import undistort_for_cli

        data = undistort_for_cli(data, not args.no_undistort, dev)
        views = cli.chosen_views(data, args.views)
        if not views:
            return cli.no_views(args, args.views)
        scene = Scene(views)
        a = eval_stats(splats, scene, antialiased=args.antialiased)
        b = eval_stats(back, scene, antialiased=args.antialiased)
        mse = torch.stack([((x.rendered.clamp(0, 1) - y.rendered.clamp(0, 1)) ** 2).mean()
                           for x, y in zip(a.samples, b.samples)]).double().cpu().numpy()
        between = float(np.mean(np.where(mse > 0, 10.0 * np.log10(1.0 / np.maximum(mse, 1e-300)), np.inf)))
        res["render"] = {"views": args.views, "num_views": len(views), "antialiased": bool(args.antialiased),
                         "original": {"psnr": a.mean_psnr(), "ssim": a.mean_ssim()},
                         "compressed": {"psnr": b.mean_psnr(), "ssim": b.mean_ssim()},
                         "psnr_between": between}
        r = res["render"]
        print(f"render ({len(views)} {args.views} views)\toriginal psnr {r['original']['psnr']:.4f} ssim "
              f"{r['original']['ssim']:.6f}\tcompressed psnr {r['compressed']['psnr']:.4f} ssim "
              f"{r['compressed']['ssim']:.6f}\tcompressed vs original psnr {between:.4f}")
    if args.export:
        with open(args.export, "wb") as f:
            f.write(blob)
    if args.json:
        cli.write_json(args.json, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
