"""The compressed PLY without a GPU: the writer and reader of brush_amd/ply.py and its numpy unpack against the independent
restatement tests/compress_ref.py, the error bounds that follow from the code widths, the float PLY left as it was, and a
committed file that pins the format."""
import os

import numpy as np
import pytest

from tests import compress_cases as Cs
from tests import compress_ref as R

F = np.float32
EPS = 2.0 ** -24  # one float32 rounding, relative


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def packed():
    """{case: (cloud, reference pack, reference unpack)}, computed once and left unchanged."""
    out = {}
    for name, make in Cs.CASES.items():
        cloud = make()
        pack = R.pack(*(cloud[k] for k in Cs.FIELDS))
        out[name] = (cloud, pack, R.unpack(pack["chunks"], pack["words"], pack["sh"]))
    return out


def _ulps(a, b):
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


# ---------------------------------------------------------------------------- writer / reader
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_writer_and_reader_are_inverse(packed, name):
    from brush_amd import ply

    _, pack, _ = packed[name]
    blob = ply.compressed_to_ply(pack["chunks"], pack["words"], pack["sh"])
    assert blob == R.write_ply(pack["chunks"], pack["words"], pack["sh"])  # the format text, written independently
    assert ply.is_compressed_ply(blob)
    chunks, words, sh = ply.load_compressed_ply(blob)
    assert chunks.dtype == np.float32 and words.dtype == np.uint32 and sh.dtype == np.uint8
    assert np.array_equal(_bits(chunks), _bits(pack["chunks"])) and chunks.shape == pack["chunks"].shape
    assert np.array_equal(words, pack["words"]) and np.array_equal(sh, pack["sh"]) and sh.shape == pack["sh"].shape
    assert ply.compressed_to_ply(chunks, words.view(np.int32), sh) == blob  # int32 words are the same bits


def test_header_names_and_order(packed):
    from brush_amd import ply

    _, pack, _ = packed["n1000_d3"]
    blob = ply.compressed_to_ply(pack["chunks"], pack["words"], pack["sh"])
    head = blob[:blob.index(b"end_header")].decode("ascii").splitlines()
    assert head[:4] == ["ply", "format binary_little_endian 1.0", "comment Exported from Brush",
                        "comment Vertical axis: y"]
    want = ["element chunk 4"] + [f"property float {p}" for p in (
        "min_x min_y min_z max_x max_y max_z min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z "
        "min_r min_g min_b max_r max_g max_b").split()]
    want += ["element vertex 1000"] + [f"property uint {p}" for p in
                                       ("packed_position", "packed_rotation", "packed_scale", "packed_color")]
    want += ["element sh 1000"] + [f"property uchar f_rest_{i}" for i in range(45)]
    assert head[4:] == want
    assert len(blob) == blob.index(b"end_header") + len("end_header\n") + 4 * 72 + 1000 * (16 + 45)
    # degree 0: no `sh` element at all
    _, pack0, _ = packed["n1000_d0"]
    head0 = ply.compressed_to_ply(pack0["chunks"], pack0["words"], pack0["sh"]).split(b"end_header")[0]
    assert b"element sh" not in head0 and b"f_rest" not in head0


def test_writer_and_reader_refuse_other_shapes(packed):
    from brush_amd import ply

    _, pack, _ = packed["n257"]
    with pytest.raises(ValueError):
        ply.compressed_to_ply(pack["chunks"], pack["words"], np.zeros((257, 12), np.uint8))  # 3K = 12: no such degree
    with pytest.raises(ValueError):
        ply.compressed_to_ply(pack["chunks"][:1], pack["words"], pack["sh"])  # 257 splats need two chunks
    with pytest.raises(ValueError):
        ply.compressed_to_ply(pack["chunks"], pack["words"].astype(np.float32), pack["sh"])
    blob = R.write_ply(pack["chunks"], pack["words"], np.zeros((257, 12), np.uint8))
    with pytest.raises(ValueError, match="9, 24 or 45"):
        ply.load_compressed_ply(blob)
    with pytest.raises(ValueError, match="9, 24 or 45"):
        ply.load_splat_from_ply(blob)
    with pytest.raises(ValueError):
        ply.load_compressed_ply(R.write_ply(pack["chunks"][:1], pack["words"], pack["sh"]))


# ---------------------------------------------------------------------------- load
@pytest.mark.parametrize("name", list(Cs.CASES))
def test_load_equals_reference_unpack(packed, name):
    """load_splat_from_ply on a compressed file: the reference unpack to the bit, raw_opacity within 4 ulp (numpy's
    logarithm against det_logf).  On the parent commit the call raises "Missing properties"."""
    from brush_amd import ply

    _, pack, want = packed[name]
    got = ply.load_splat_from_ply(R.write_ply(pack["chunks"], pack["words"], pack["sh"]))
    assert sorted(got) == sorted(Cs.FIELDS)
    for k in Cs.FIELDS:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        if k == "raw_opacity":
            assert np.isfinite(got[k]).all()
            print(name, "raw_opacity ulps", _ulps(got[k], want[k]))
            assert _ulps(got[k], want[k]) <= 4
        else:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k


def test_every_opacity_code_loads_finite_and_close():
    """All 256 opacity codes (the cases reach only some): finite at 0 and 255, within 4 ulp of det_logf."""
    from brush_amd import ply

    words = np.zeros((256, 4), np.uint32)
    words[:, 3] = np.arange(256)
    chunks = np.zeros((1, 18), F)
    chunks[0, 3:6] = chunks[0, 9:12] = chunks[0, 15:18] = 1.0
    sh = np.zeros((256, 0), np.uint8)
    got = ply.load_splat_from_ply(R.write_ply(chunks, words, sh))["raw_opacity"]
    want = R.unpack(chunks, words, sh)["raw_opacity"]
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert got[0] == got[0] and got[0] < -6.0 and got[255] > 6.0 and (np.diff(got) > 0).all()
    print("worst ulps over the codes", _ulps(got, want))
    assert _ulps(got, want) <= 4


# ---------------------------------------------------------------------------- error bounds
def test_round_trip_error_bounds(packed):
    """Reference pack -> reference unpack against the input, per chunk.  The bounds follow from the code widths:

    * position and scale, b bits on an extent E = hi - lo >= 1e-5: the code is the nearest of 2^b - 1 steps of
      E / (2^b - 1), so the decoded value is within half a step, plus float32 roundings: norm makes two (the difference
      and the quotient), the code's rounding argument two, the decode five (t, 1 - t, two products, the sum), each at
      most 2^-24 of a term no larger than M = max(|lo|, |hi|) + E.  A rounding can at worst move a value that sits on
      a code boundary to the other neighbour, which stays inside half a step plus the same slack: 16 * 2^-24 * M covers
      them.  Scales are compared after the clamp to [-20, 20] the packer applies.
    * an extent below 1e-5 (norm's third branch) decodes to lo or hi: the error is below the extent, 1e-5.
    * colour: the same with 8 bits on c = f_dc * 0.28209479 + 0.5, then divided by 0.28209479: half a step of
      E_c / 255 / 0.28209479 in f_dc, with the slack taken on |c| <= M_c and scaled alike.
    * rotation: a stored component a_i in [-0.70710678, 0.70710678] goes through a_i * 0.70710678 + 0.5 onto 1023
      steps and comes back times 1.41421356: half a step is 1.41421356 / 1023 / 2 (slack: 16 * 2^-24).  The input is
      normalised and sign-aligned in float64 first; the largest component is not stored and not bounded here.
    * SH: byte = floor((v / 8 + 0.5) * 256) decodes to the centre of its cell of width 8 / 256, so half a cell,
      8 / 256 / 2, for v inside [-4, 4) (slack: 16 * 2^-24 * 4).
    """
    worst = {}
    for name in ("n1000_d3", "n257", "n1", "flat_axis", "ranges", "tiny_extent", "quaternions"):
        cloud, pack, back = packed[name]
        order = pack["order"]
        n = len(order)
        src = {k: cloud[k][order].astype(np.float64) for k in Cs.FIELDS}
        src["log_scales"] = np.clip(src["log_scales"], -20.0, 20.0)
        for j in range(pack["chunks"].shape[0]):
            rows = slice(256 * j, min(256 * j + 256, n))
            ch = pack["chunks"][j].astype(np.float64)
            for key, base, bits in (("means", 0, (11, 10, 11)), ("log_scales", 6, (11, 10, 11))):
                for axis in range(3):
                    lo, hi = ch[base + axis], ch[base + 3 + axis]
                    extent = hi - lo
                    err = np.abs(back[key][rows, axis].astype(np.float64) - src[key][rows, axis]).max()
                    slack = 16 * EPS * (max(abs(lo), abs(hi)) + extent)
                    bound = 1e-5 if F(hi) - F(lo) < F(1e-5) else 0.5 * extent / (2 ** bits[axis] - 1) + slack
                    assert err <= bound, (name, key, j, axis, err, bound)
                    if extent >= 1e-5:
                        worst[key] = max(worst.get(key, 0.0), (err - slack) / (0.5 * extent / (2 ** bits[axis] - 1)))
            for c in range(3):
                lo, hi = ch[12 + c], ch[15 + c]
                extent = hi - lo
                err = np.abs(back["sh_coeffs"][rows, 0, c].astype(np.float64) - src["sh_coeffs"][rows, 0, c]).max()
                slack = 16 * EPS * (max(abs(lo), abs(hi)) + extent)
                bound = (1e-5 if F(hi) - F(lo) < F(1e-5) else 0.5 * extent / 255 + slack) / 0.28209479
                assert err <= bound, (name, "colour", j, c, err, bound)
        q = src["rotation"]
        length = np.sqrt((q * q).sum(1, keepdims=True))
        ok = (length[:, 0] > 1e-15) & (length[:, 0] < 1e15)  # the others pack as the identity (directed test below)
        q = q[ok] / length[ok]
        got = back["rotation"][ok].astype(np.float64)
        big = (pack["words"][ok, 1] >> 30).astype(np.int64)
        q = q * np.sign(q[np.arange(len(q)), big])[:, None]
        stored = np.ones_like(q, dtype=bool)
        stored[np.arange(len(q)), big] = False
        err = np.abs(got - q)[stored].max()
        assert err <= 1.41421356 / 1023 / 2 + 16 * EPS, (name, "rotation", err)
        worst["rotation"] = max(worst.get("rotation", 0.0), err / (1.41421356 / 1023 / 2))
        if back["sh_coeffs"].shape[1] > 1:
            rest, dec = src["sh_coeffs"][:, 1:], back["sh_coeffs"][:, 1:].astype(np.float64)
            inside = (rest >= -4.0) & (rest < 4.0)
            err = np.abs(dec - rest)[inside].max()
            assert err <= 8 / 256 / 2 + 16 * EPS * 4, (name, "sh", err)
            # outside the range the byte saturates: the decoded value is the first or the last cell's centre
            assert (dec[rest < -4.0] == -4.0 + 1 / 64).all() and (dec[rest >= 4.0] == 4.0 - 1 / 64).all()
            worst["sh"] = max(worst.get("sh", 0.0), err / (8 / 256 / 2))
    print("worst error as a fraction of the half step:", worst)


def test_directed_quaternions_and_ranges(packed):
    """What the directed rows must give, read off the reference's words (the GPU test holds the kernels to them)."""
    cloud, pack, back = packed["quaternions"]
    by_input = np.argsort(pack["order"])  # packed row of every input splat
    words = pack["words"][by_input, 1]
    big = words >> 30
    assert big[:8].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]     # each component largest, either sign
    assert (words[0:8:2] & 0x3FFFFFFF != words[1:8:2] & 0x3FFFFFFF).all()  # the sign flip negates the others
    assert big[8:12].tolist() == [0, 0, 0, 0]               # |w| = |x|: the first index
    assert big[12] == 0 and big[13] == 0 and big[14] == 1   # four-way tie, and |x| = |z|
    identity = 0 << 30 | 512 << 20 | 512 << 10 | 512        # (1, 0, 0, 0): unorm(0.5, 10) = floor(512)
    assert words[19:23].tolist() == [identity] * 4          # zero, signed zero, overflowing and underflowing norms
    assert words[23] == identity and big[24] == 3 and big[25] == 2
    rot = back["rotation"][by_input]
    assert rot[19, 0] > 0.9999 and np.abs(rot[19, 1:]).max() < 1e-3  # code 512 is the cell beside zero
    for row in (16, 17, 18):  # not normalised: the decoded rotation is the normalised one
        q = cloud["rotation"][row].astype(np.float64)
        q = q / np.linalg.norm(q)
        q = q * np.sign(q[np.argmax(np.abs(q))])
        assert np.abs(rot[row] - q).max() < 2e-3, row

    cloud, pack, back = packed["ranges"]
    by_input = np.argsort(pack["order"])
    alpha = pack["words"][by_input, 3] & 0xFF
    assert alpha[:6].tolist() == [255, 0, 128, 128, 255, 0]  # +-30, +-0, beyond the exponential's range
    assert np.isfinite(back["raw_opacity"]).all()
    scales = back["log_scales"][by_input]
    assert scales.min() >= -20.0 and scales.max() <= 20.0 and scales[0, 0] == -20.0 and scales[1, 0] == 20.0
    # -0 and +0 among the means pack alike
    assert np.array_equal(pack["words"][by_input[0], 0], pack["words"][by_input[1], 0])
    _, same, _ = packed["signed_zero_means"]
    assert np.array_equal(same["order"], np.arange(40)) and not same["chunks"][0, :6].any()
    assert not np.signbit(same["chunks"][0, :6]).any()
    _, equal, _ = packed["equal_means"]
    assert np.array_equal(equal["order"], np.arange(300))


# ---------------------------------------------------------------------------- existing behaviour
def test_float_ply_is_written_and_read_as_before():
    """splat_to_ply's bytes are the header and rows written out here by hand, load_splat_from_ply returns the arrays
    to the bit, and an export name that does not end in .compressed.ply gets exactly those bytes."""
    import torch

    from brush_amd import Splats, ply
    from brush_amd.compress import ply_bytes_for

    c = Cs.cloud(37, 2, 91)
    blob = ply.splat_to_ply(c["means"], c["log_scales"], c["rotation"], c["raw_opacity"], c["sh_coeffs"])
    names = ["x", "y", "z", "scale_0", "scale_1", "scale_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3", "f_dc_0",
             "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(24)]
    head = "\n".join(["ply", "format binary_little_endian 1.0", "comment Exported from Brush",
                      "comment Vertical axis: y", "element vertex 37"] + [f"property float {p}" for p in names] +
                     ["end_header"]) + "\n"
    rows = np.concatenate([c["means"], c["log_scales"], c["raw_opacity"][:, None], c["rotation"], c["sh_coeffs"][:, 0],
                           c["sh_coeffs"][:, 1:].transpose(0, 2, 1).reshape(37, 24)], axis=1).astype("<f4")
    assert blob == head.encode("ascii") + rows.tobytes()
    assert not ply.is_compressed_ply(blob)
    got = ply.load_splat_from_ply(blob)
    for k in Cs.FIELDS:
        assert np.array_equal(_bits(got[k]), _bits(c[k])), k
    t = lambda a: torch.from_numpy(a)
    splats = Splats(t(c["means"]), t(c["sh_coeffs"]), t(c["rotation"]), t(c["raw_opacity"]), t(c["log_scales"]))
    assert splats.to_ply() == blob and ply_bytes_for(splats, "out.ply") == blob
    assert ply_bytes_for(splats, "out.compressed.ply.bak") == blob
    with pytest.raises(ValueError, match="runs on the device"):
        splats.to_compressed_ply()
    with pytest.raises(ValueError, match="runs on the device"):
        ply_bytes_for(splats, "out.compressed.ply")


def test_chunk_element_without_packed_words_is_still_refused():
    from brush_amd import ply

    head = "\n".join(["ply", "format binary_little_endian 1.0", "element chunk 1"] +
                     [f"property float {p}" for p in R.CHUNK_PROPS] +
                     ["element vertex 2", "property uint packed_rotation", "property uint packed_scale",
                      "property uint packed_color", "end_header"]) + "\n"
    blob = head.encode("ascii") + np.zeros(18, "<f4").tobytes() + np.zeros(6, "<u4").tobytes()
    assert not ply.is_compressed_ply(blob)
    with pytest.raises(ValueError, match="Missing properties"):
        ply.load_splat_from_ply(blob)
    with pytest.raises(ValueError):
        ply.load_compressed_ply(blob)
    with pytest.raises(ValueError):
        ply.is_compressed_ply(b"not a ply at all")


def test_cpu_import_of_a_compressed_file(packed):
    """Splats.from_ply on a CPU device goes through numpy and ends in norm_rotations()."""
    import torch

    from brush_amd import Splats

    _, pack, want = packed["n257"]
    splats = Splats.from_ply(R.write_ply(pack["chunks"], pack["words"], pack["sh"]), torch.device("cpu"))
    assert splats.num_splats() == 257 and tuple(splats.sh_coeffs.shape) == (257, 4, 3)
    assert np.array_equal(_bits(splats.means.detach().numpy()), _bits(want["means"]))
    assert np.array_equal(_bits(splats.sh_coeffs.detach().numpy()), _bits(want["sh_coeffs"]))
    length = np.linalg.norm(splats.rotation.detach().numpy().astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6


# ---------------------------------------------------------------------------- the ABI's argument checks, no device
def test_entry_points_check_their_arguments():
    import ctypes as C

    from brush_amd import _lib

    lib = _lib.lib()
    for name in ("brush_splat_pack_workspace_size", "brush_splat_pack_keys", "brush_splat_pack", "brush_splat_unpack"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)
    size = C.c_size_t()
    assert lib.brush_splat_pack_workspace_size(1000, C.byref(size)) == 0 and size.value >= 4 * 8 * 4 + 6 * 4
    assert lib.brush_splat_pack_workspace_size(0, C.byref(size)) == -1
    assert lib.brush_splat_pack_workspace_size(1000, None) == -1
    p = 4096  # a well-aligned non-NULL address: every call below must return before it touches memory
    assert lib.brush_splat_pack_keys(p, p, p, p, p, 10, 4, p, p, p, p, 1 << 20, None) == -1   # no degree 4
    assert lib.brush_splat_pack_keys(p, p, p, p, p, 0, 3, p, p, p, p, 1 << 20, None) == -1
    assert lib.brush_splat_pack_keys(p, p, p, p, None, 10, 3, p, p, p, p, 1 << 20, None) == -1
    assert lib.brush_splat_pack_keys(p, p, p, p, p, 10, 3, p, p, p, p, 8, None) == -2          # workspace too small
    assert lib.brush_splat_pack(p, p, p, p, p, 10, 1, 2, p, p, p, p, None) == -1              # more bands than it has
    assert lib.brush_splat_pack(p, p, p + 4, p, p, 10, 1, 1, p, p, p, p, None) == -1          # rotation rows: 16 bytes
    assert lib.brush_splat_pack(p, p, p, p, p, 10, 1, 1, p, p, p + 8, p, None) == -1          # words: 16 bytes
    assert lib.brush_splat_pack(p, p, p, p, p, 10, 1, 1, p, p, p, None, None) == -1           # SH bytes wanted
    assert lib.brush_splat_unpack(p, p, p, 10, 4, p, p, p, p, p, None) == -1
    assert lib.brush_splat_unpack(p, p, None, 10, 2, p, p, p, p, p, None) == -1
    assert lib.brush_splat_unpack(p, p, p, 10, 3, p, p, p, p, p + 4, None) == -1              # degree 3 rows: 16 bytes


# ---------------------------------------------------------------------------- golden file
def golden_cloud():
    """The cloud of tests/golden/compressed_small.ply: 300 splats, SH degree 1, from this seed."""
    return Cs.cloud(300, 1, 20261021)


def test_golden_file_pins_the_format(golden_dir):
    """tests/golden/compressed_small.ply was written once by the reference packer from golden_cloud(): the reference
    still writes those bytes, and the product loads them to the reference unpack."""
    from brush_amd import ply

    with open(os.path.join(golden_dir, "compressed_small.ply"), "rb") as f:
        blob = f.read()
    cloud = golden_cloud()
    pack = R.pack(*(cloud[k] for k in Cs.FIELDS))
    assert blob == R.write_ply(pack["chunks"], pack["words"], pack["sh"])
    assert len(blob) < 9000
    want = R.unpack(pack["chunks"], pack["words"], pack["sh"])
    got = ply.load_splat_from_ply(blob)
    for k in Cs.FIELDS:
        if k == "raw_opacity":
            assert _ulps(got[k], want[k]) <= 4
        else:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    chunks, words, sh = ply.load_compressed_ply(blob)
    assert chunks.shape == (2, 18) and words.shape == (300, 4) and sh.shape == (300, 9)
