"""GPU checks of the compressed splat kernels (brush_splat_pack_keys / brush_splat_pack / brush_splat_unpack through
brush_amd/compress.py) against the independent restatement tests/compress_ref.py, bit for bit, on the directed inputs of
tests/compress_cases.py; the device round trip against the numpy path; SH truncation; the refusals; the command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import compress_cases as Cs
from tests import compress_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def reference():
    """{case: (cloud, reference pack, reference unpack)}, computed once and left unchanged."""
    out = {}
    for name, make in Cs.CASES.items():
        cloud = make()
        pack = R.pack(*(cloud[k] for k in Cs.FIELDS))
        out[name] = (cloud, pack, R.unpack(pack["chunks"], pack["words"], pack["sh"]))
    return out


def _splats(cloud, dev):
    import torch

    from brush_amd import Splats

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return Splats(t(cloud["means"]), t(cloud["sh_coeffs"]), t(cloud["rotation"]), t(cloud["raw_opacity"]),
                  t(cloud["log_scales"]))


def _host(packed):
    """(order, chunks bits, words, sh) of a PackedSplats as numpy arrays."""
    return (packed.order.cpu().numpy(), packed.chunks.cpu().numpy().view(np.uint32),
            packed.words.cpu().numpy().view(np.uint32), packed.sh.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _param(splats, k):
    return getattr(splats, k).detach().cpu().numpy()


# ---------------------------------------------------------------------------- pack and unpack
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_pack_and_unpack_equal_the_reference_bitwise(dev, reference, name):
    from brush_amd.compress import PackedSplats, morton_order, pack_splats

    cloud, want, want_back = reference[name]
    splats = _splats(cloud, dev)
    packed = pack_splats(splats)
    order, chunks, words, sh = _host(packed)
    n = len(cloud["means"])
    assert packed.sh_degree == want["sh_degree"] and packed.num_splats == n
    assert packed.nbytes == 72 * -(-n // 256) + n * (16 + want["sh"].shape[1])
    assert order.dtype == np.int32 and np.array_equal(order, want["order"])
    assert np.array_equal(morton_order(splats.means.detach()).cpu().numpy(), want["order"])
    assert chunks.shape == want["chunks"].shape and np.array_equal(chunks, _bits(want["chunks"]))
    bad = np.nonzero((words != want["words"]).any(1))[0]
    assert bad.size == 0, (bad[:8], words[bad[:8]], want["words"][bad[:8]])  # the opacity byte included
    assert sh.shape == want["sh"].shape and np.array_equal(sh, want["sh"])
    # two runs give equal bytes, in the file too
    again = pack_splats(splats)
    for a, b in zip(_host(again), (order, chunks, words, sh)):
        assert np.array_equal(a, b)
    blob = packed.to_ply()
    assert blob == again.to_ply() == R.write_ply(want["chunks"], want["words"], want["sh"])
    # unpack, from the packed arrays and from the file
    for source in (packed, PackedSplats.from_ply(blob, dev)):
        back = source.unpack()
        for k in Cs.FIELDS:
            got = _param(back, k)
            assert got.shape == want_back[k].shape, k
            assert np.array_equal(_bits(got), _bits(want_back[k])), (name, k)


@pytest.mark.parametrize("name", ["n257", "n1000_d3", "quaternions", "ranges"])
def test_round_trip_on_the_device_equals_the_numpy_path(dev, reference, name):
    """Splats.from_ply on the device (packed arrays uploaded, brush_splat_unpack) against the numpy path
    (ply.load_splat_from_ply), both ending in norm_rotations() on the same device: exact, raw_opacity within 4 ulp.
    The import on a CPU device is the numpy path with torch's CPU normalisation: exact again except the rotations,
    where the two devices' torch kernels may order the four-term sum of squares differently (each order carries at
    most three roundings, the square root halves their difference, then one rounding each for the root and the
    quotient: 8 ulp covers it)."""
    import torch

    from brush_amd import Splats
    from brush_amd.ply import load_splat_from_ply

    cloud, _, _ = reference[name]
    blob = _splats(cloud, dev).to_compressed_ply()
    on_device = Splats.from_ply(blob, dev)
    d = load_splat_from_ply(blob)
    via_numpy = _splats(d, dev)
    via_numpy.norm_rotations()
    on_host = Splats.from_ply(blob, torch.device("cpu"))
    for k in Cs.FIELDS:
        a, b, c = _param(on_device, k), _param(via_numpy, k), _param(on_host, k)
        if k == "raw_opacity":
            print(name, "raw_opacity ulps", _ulps(a, b))
            assert _ulps(a, b) <= 4 and _ulps(a, c) <= 4  # numpy's logarithm against det_logf
        else:
            assert np.array_equal(_bits(a), _bits(b)), (name, k)
            if k == "rotation":
                assert _ulps(a, c) <= 8, (name, _ulps(a, c))
            else:
                assert np.array_equal(_bits(a), _bits(c)), (name, k)
    length = np.linalg.norm(_param(on_device, "rotation").astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6
    # a file name decides the form of an export
    from brush_amd.compress import ply_bytes_for

    assert ply_bytes_for(_splats(cloud, dev), "a.compressed.ply") == blob
    assert ply_bytes_for(_splats(cloud, dev), "a.ply") == _splats(cloud, dev).to_ply()


@pytest.mark.parametrize("name,degrees", [("n1000_d3", (0, 1, 2)), ("n1000_d2", (0, 1)), ("n257", (0,))])
def test_sh_truncation_keeps_the_words_and_the_leading_bands(dev, reference, name, degrees):
    from brush_amd.compress import pack_splats

    cloud, want, _ = reference[name]
    splats = _splats(cloud, dev)
    full_k = want["sh"].shape[1] // 3
    for degree in degrees:
        order, chunks, words, sh = _host(pack_splats(splats, sh_degree=degree))
        k = (degree + 1) ** 2 - 1
        assert np.array_equal(order, want["order"]) and np.array_equal(chunks, _bits(want["chunks"]))
        assert np.array_equal(words, want["words"])
        assert sh.shape == (len(order), 3 * k)
        n = len(order)
        lead = want["sh"].reshape(n, 3, full_k)[:, :, :k].reshape(n, 3 * k)  # channel-major: the first k of each
        assert np.array_equal(sh, lead)
        ref = R.pack(*(cloud[f] for f in Cs.FIELDS), sh_degree=degree)
        assert np.array_equal(sh, ref["sh"])
    with pytest.raises(ValueError, match="sh_degree"):
        pack_splats(splats, sh_degree=want["sh_degree"] + 1)
    with pytest.raises(ValueError, match="sh_degree"):
        splats.to_compressed_ply(sh_degree=want["sh_degree"] + 1)


def test_refusals(dev):
    import torch

    from brush_amd import Splats
    from brush_amd.compress import pack_splats

    nan = Cs.NAN_CASE()
    packed = pack_splats(_splats(nan, dev))  # packing itself is launches only: the flag is read with the arrays
    with pytest.raises(ValueError, match="non-finite"):
        packed.to_ply()
    with pytest.raises(ValueError, match="non-finite"):
        _splats(nan, dev).to_compressed_ply()
    inf = Cs.cloud(300, 0, 31)
    inf["log_scales"][299, 2] = np.float32(np.inf)
    with pytest.raises(ValueError, match="non-finite"):
        _splats(inf, dev).to_compressed_ply()
    c = Cs.cloud(5, 1, 30)
    t = lambda a: torch.from_numpy(a)
    cpu = Splats(t(c["means"]), t(c["sh_coeffs"]), t(c["rotation"]), t(c["raw_opacity"]), t(c["log_scales"]))
    with pytest.raises(ValueError, match="runs on the device"):
        cpu.to_compressed_ply()
    with pytest.raises(ValueError, match="runs on the device"):
        pack_splats(cpu)
    odd = Cs.cloud(5, 1, 30)
    odd["sh_coeffs"] = np.zeros((5, 25, 3), np.float32)  # degree 4: the layout has no such coefficient count
    with pytest.raises(ValueError, match="SH degrees 0 to 3"):
        _splats(odd, dev).to_compressed_ply()
    # a finite cloud right after: nothing of the refused ones lingers
    ok = Cs.cloud(300, 0, 31)
    assert len(_splats(ok, dev).to_compressed_ply()) > 300 * 16


# ---------------------------------------------------------------------------- the command line
def _write_scene(root, dev, splats, w=64, h=64, n=3):
    """A three-view NeRF-synthetic tree (train views only) of renders of `splats`."""
    import torch

    from brush_amd.dataset import nerf_camera
    from tests import eval_data as E

    fovx = 0.6911112070083618
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    frames = []
    for i in range(n):
        ang = 2.0 * math.pi * i / n + 0.1
        c2w = E.look_at_gl((4.0 * math.cos(ang), 4.0 * math.sin(ang), 1.0)).astype(np.float32).astype(np.float64)
        with torch.no_grad():
            pred, _ = splats.render(nerf_camera(c2w, fovx, w, h), (w, h), False)
        img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
        with open(os.path.join(root, "train", f"r_{i}.png"), "wb") as f:
            f.write(E.png_bytes(img))
        frames.append({"file_path": f"./train/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


def test_command_line(dev, tmp_path):
    """python -m brush_amd.compress in a fresh child process on a 300-splat file and a three-view dataset: finite
    PSNR values, fewer bytes, an export that loads.  No PSNR threshold: nothing here has measured one."""
    import torch

    from brush_amd import Splats
    from brush_amd.ply import is_compressed_ply, load_splat_from_ply

    splats = Splats.from_random_config(300, 1, (np.full(3, -0.8), np.full(3, 0.8)), np.random.default_rng(12), dev)
    with torch.no_grad():
        splats.log_scales.fill_(math.log(0.1))
        splats.raw_opacity.fill_(math.log(0.8 / 0.2))
        splats.sh_coeffs[:, 1:] = torch.from_numpy(
            np.random.default_rng(13).uniform(-0.3, 0.3, (300, 3, 3)).astype(np.float32)).to(dev)
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(splats.to_ply())
    scene = _write_scene(str(tmp_path / "scene"), dev, splats)
    out, out_json = str(tmp_path / "cloud.compressed.ply"), str(tmp_path / "report.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.compress", src, "--dataset", scene, "--views", "train",
                        "--export", out, "--json", out_json], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    print(r.stdout)
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("splats\t300") and lines[1].startswith("bytes\traw ")
    assert lines[2].startswith("max |round trip - original|") and lines[3].startswith("render (3 train views)")
    with open(out_json) as f:
        res = json.load(f)
    assert res["num_splats"] == 300 and res["sh_degree"] == 1
    assert res["bytes_raw"] == 300 * 4 * 23 and res["bytes_compressed"] == 2 * 72 + 300 * 25
    assert res["bytes_compressed"] < res["bytes_raw"]
    render = res["render"]
    for v in (render["original"]["psnr"], render["compressed"]["psnr"], render["psnr_between"],
              render["original"]["ssim"], render["compressed"]["ssim"]):
        assert isinstance(v, float) and math.isfinite(v), render
    assert render["num_views"] == 3
    assert all(math.isfinite(v) for v in res["max_abs_error"].values()) and "sh_rest" in res["max_abs_error"]
    assert is_compressed_ply(out) and os.path.getsize(out) == res["file_bytes_compressed"]
    d = load_splat_from_ply(out)
    assert d["means"].shape == (300, 3) and d["sh_coeffs"].shape == (300, 4, 3)
    back = Splats.from_ply(out, dev)
    assert back.num_splats() == 300
    # the positions come back within half a step of the chunks' extents (1.6 / 1023 / 2 at most on the 10-bit axis, plus roundings)
    row_of = np.argsort(R.morton_order(_param(splats, "means")))  # the packed row of every input splat
    assert np.abs(_param(back, "means")[row_of] - _param(splats, "means")).max() < 1.6 / 1023 / 2 + 1e-5
