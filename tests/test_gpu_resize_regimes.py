"""The pyramid resamplers at every dispatch switch, exactly (pytest -m gpu).

brush_amd/csrc/resize.hip picks its code path from the shapes alone: two area kernels, 64 or 256 lanes, strips of 1 to 8
output rows, rows staged whole / several per barrier round / one row in chunks, a 32- or 64-bit accumulator, an integer
kernel of one or several rounds.  Each case of tests/resize_cases.py (shapes and switch there) sits on one side of one
of those switches; tests/test_pyramid_cpu.py asserts that from a restatement of the dispatch.  Here every case runs
through the C ABI in a 4096-byte guard band, on six images (random, zeros, full, ramp, coin, coin + 254), for RGB and
RGBA, and has to equal tests/pyramid_ref.py's area_resize_integral byte for byte: the function is defined in integers,
so there is no tolerance.  The coin images (every byte 0 or 1) make every output a rounding decision at D / 2; "ties"
counts the outputs of the coin image that sit exactly on it (S mod D == D / 2), RGB / RGBA.  "s" is the whole test on
one MI355X, both channel counts, the host references included (six at a time on threads).

| case                  | kernel, lanes (RGB / RGBA)                         | ties            | s      |
|-----------------------|----------------------------------------------------|-----------------|--------|
| lanes_64_at_1023      | general 64: 7 rows a round / 5 rows a round        | 961 / 1375      | 0.27   |
| lanes_256_at_1024     | general 256                                        | 777 / 997       | 0.02   |
| small_general         | general 64, 7 rows a round                         | 3 / 8           | 0.02   |
| workload_1080p        | general 256, 3 rows a round                        | 0 / 0           | 0.32   |
| strip_2               | general 256, strips of 2                           | 1583 / 2070     | 0.15   |
| strip_2_ragged        | general 256, strips of 2                           | 2487 / 3292     | 0.33   |
| strip_3               | general 256, strips of 3                           | 2369 / 3080     | 0.34   |
| strip_7_ragged        | general 256, strips of 7                           | 6427 / 8463     | 0.78   |
| strip_8               | general 256, strips of 8                           | 6119 / 8278     | 0.63   |
| strip_8_capped_ragged | general 256, strips of 8                           | 12439 / 16846   | 1.52   |
| chunked_64_lanes      | general 64: 2 chunks / 3 chunks                    | 21 / 32         | < 0.01 |
| chunked_63_lanes      | general 64: 2 chunks / 3 chunks                    | 0 / 0           | < 0.01 |
| fx31_256_lanes        | int 256: slot 1489 / slot 1985                     | 0 / 0           | 0.32   |
| fx32_256_lanes        | int 256, slot 1537 / general 256, 2 chunks         | 110410 / 146118 | 0.33   |
| chunked_256_lanes     | general 256: 1 rows a round / 2 chunks             | 0 / 0           | 0.34   |
| fx127_64_lanes        | int 64: slot 1525, 2 rounds / slot 2033, 2 rounds  | 10 / 8          | < 0.01 |
| fx128_64_lanes        | int 64, slot 1537, 2 rounds / general 64, 2 chunks | 10 / 14         | < 0.01 |
| fx85_batch_2_or_1     | int 64: slot 1021 / slot 1361, 2 rounds            | 22 / 28         | < 0.01 |
| fy17_two_rounds       | int 64: slot 13, 2 rounds / slot 16, 2 rounds      | 0 / 0           | < 0.01 |
| 15x17_two_rounds      | int 64: slot 4, 2 rounds / slot 5, 2 rounds        | 0 / 0           | < 0.01 |
| fy255_16_rounds       | int 64, slot 2, 16 rounds                          | 0 / 0           | < 0.01 |
| block_256_square      | int 64: slot 4 / slot 5                            | 0 / 0           | < 0.01 |
| block_256_flat        | int 64: slot 7 / slot 9                            | 0 / 0           | < 0.01 |
| block_272             | general 64                                         | 0 / 0           | < 0.01 |
| block_1024            | general 64                                         | 0 / 0           | < 0.01 |
| identity_row          | int 64: slot 13 / slot 17                          | 0 / 0           | < 0.01 |
| row_to_pixel          | general 64: 2 chunks / 3 chunks                    | 0 / 0           | 0.02   |
| column_to_pixel       | general 64                                         | 0 / 0           | 0.25   |
| identity_column       | int 256, slot 2                                    | 0 / 0           | 0.18   |
| row_16384_to_16383    | general 64, 4 rows a round                         | 12406 / 16569   | < 0.01 |
| acc32_strips_of_8     | general 256, strips of 8, 32-bit (RGB)             |                 | 0.85   |
| acc32_chunked         | general 64, 2 chunks, 32-bit (RGB)                 |                 | "      |
| acc64_strips_of_8     | general 256, strips of 8, 64-bit (RGB)             |                 | 0.88   |
| acc64_chunked         | general 64, 2 chunks, 64-bit (RGB)                 |                 | "      |

The two 16.8 M-pixel sources (D = 16384 x 1026: 255 D + D / 2 = 4 294 950 912, the 32-bit accumulator's ceiling, reached
by `full`; D = 16384 x 1027: the first 64-bit one) run as RGB.  area_resize_integral costs the host 1.5 s per image at
-> (8191,513), and the -> (3,2) shape a third of a second of two workgroups per call, so this group is cut to what the
switch needs to keep the module no slower than tests/test_gpu_pyramid.py: -> (3,2) runs a random image against
area_resize_integral; -> (8191,513) runs `full` and a separable image a[r] b[s] (c + 1), the construction of
test_gpu_pyramid.py's 64-bit test, against the factored reference pyramid_ref.area_resize_separable (which
tests/test_pyramid_cpu.py pins to the two other references).

Besides: three byte offsets of the source (the staging `pad`) on general, chunked and integer cases; every block sum the
integer kernel's multiply-high division can see, at 64 and at 256 lanes (tests/resize_cases.py: SWEEP; three of the ten
block shapes have no 256-lane shape within the memory bound, see there); the same bits twice and from a replayed graph
for the chunked 256-lane case and a strip-of-8 case; the nearest pick at sides near 16384, with NaN payloads, and from
a 2-mod-4 address.

Seconds on the same MI355X: the three offsets 0.30, the ten block shapes 1.30; the whole module 12.2 in a process of its
own, tests/test_gpu_pyramid.py 11.5 in the same session.

Everything held at the first run on the device: no kernel change came out of this module.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import pyramid_ref as P
from tests import resize_cases as RC
from tests.test_gpu_pyramid import GUARD, _as_bits, _depth_map

pytestmark = pytest.mark.gpu

PAD = 4096


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=7) as ex:  # a case's references, side by side (numpy releases the lock)
        yield ex


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _upload(dev, a, offset=0):
    """The bytes of `a` on the device, `offset` bytes into their allocation: (tensor to keep alive, data pointer)."""
    import torch

    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if offset == 0:
        t = torch.from_numpy(flat).to(dev)
    else:
        host = np.zeros(offset + flat.size, np.uint8)
        host[offset:] = flat
        t = torch.from_numpy(host).to(dev)
    return t, t.data_ptr() + offset


def _guarded(dev, nbytes, call):
    """Runs call(dst pointer) on nbytes of a buffer with PAD guard bytes on both sides; the nbytes, as host uint8."""
    import torch

    buf = torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device=dev)
    assert call(buf.data_ptr() + PAD) == 0
    host = buf.cpu().numpy()
    assert (host[:PAD] == GUARD).all() and (host[PAD + nbytes:] == GUARD).all()
    return host[PAD:PAD + nbytes]


def _area(dev, img, ow, oh, offset=0, src=None):
    """brush_area_resize_u8 of the host image through the C ABI, inside the guard band: uint8 [oh,ow,c].  `src` is the
    image's device pointer where the caller has uploaded it already."""
    from brush_amd import _lib

    h, w, c = img.shape
    keep = None
    if src is None:
        keep, src = _upload(dev, img, offset)
    out = _guarded(dev, ow * oh * c,
                   lambda dst: _lib.lib().brush_area_resize_u8(src, w, h, c, dst, ow, oh, _stream()))
    del keep
    return out.reshape(oh, ow, c)


def _assert_same(got, ref, what):
    if not np.array_equal(got, ref):
        first = tuple(int(v) for v in np.argwhere(got != ref)[0])
        raise AssertionError(f"{what}: {int((got != ref).sum())} bytes differ, the first at (Y, X, c) = {first}: "
                             f"{int(got[first])} for {int(ref[first])}")


def _reference_and_ties(img, ow, oh):
    """area_resize_integral(img, ow, oh) in its two steps, with the exact ties of its sums counted in between."""
    D = img.shape[0] * img.shape[1]
    S = P.area_sums_integral(img, ow, oh)
    ties = RC.tie_count(S, D)
    return P.round_sums(S, D), ties


# ---------------------------------------------------------------------------- 1. every switch, exactly
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_equals_the_reference(dev, pool, name, channels):
    w, h, ow, oh, _ = RC.expected(name, channels)
    seed = RC.seed_of(name, channels)
    imgs = dict(zip(RC.PATTERNS, pool.map(lambda p: RC.image(w, h, channels, p, seed), RC.PATTERNS)))
    want = {p: pool.submit(_reference_and_ties if p == "coin" else P.area_resize_integral, img, ow, oh)
            for p, img in imgs.items()}
    got = {p: _area(dev, img, ow, oh) for p, img in imgs.items()}
    coin, ties = want["coin"].result()
    for p in RC.PATTERNS:
        _assert_same(got[p], coin if p == "coin" else want[p].result(), f"{name} x{channels} {p}")
    assert ties == RC.TIES[name][channels - 3], (name, channels, ties)
    assert np.array_equal(got["coin254"], got["coin"] + np.uint8(254))  # a shift by a constant shifts every output


# ---------------------------------------------------------------------------- 2. source alignment
@pytest.mark.parametrize("offset", [1, 5, 15])
def test_source_at_a_byte_offset(dev, pool, offset):
    """General (64 and 256 lanes), chunked (64 and 256 lanes) and integer (one and several rounds) cases with the source
    1, 5 and 15 bytes into its allocation: rows' first bytes then sit at other remainders of 16 than from offset 0."""
    work = []
    for name in ("small_general", "lanes_256_at_1024", "chunked_64_lanes", "chunked_256_lanes", "fy17_two_rounds",
                 "fx127_64_lanes"):
        for channels in (3, 4):
            w, h, ow, oh, _ = RC.expected(name, channels)
            img = RC.image(w, h, channels, "random", RC.seed_of(name, channels) + offset)
            want = pool.submit(P.area_resize_integral, img, ow, oh)
            work.append((f"{name} x{channels} at +{offset}", want, _area(dev, img, ow, oh, offset)))
    for what, want, got in work:
        _assert_same(got, want.result(), what)


# ---------------------------------------------------------------------------- 3. the multiply-high division
@pytest.mark.parametrize("fx,fy,small,big", RC.SWEEP)
def test_integer_kernel_divides_every_block_sum(dev, pool, fx, fy, small, big):
    """Every sum S = 0 .. 255 fx fy of an fy x fx block, in every channel, in shuffled order: all the inputs
    (2 S + n) magic >> 32 can see, at 64 lanes and (where such a shape exists) at 256."""
    import torch

    n = fx * fy
    shared, work = None, []
    for size in (small, big):
        if size is None:
            continue
        ow, oh = size
        img, sums, shared = RC.block_sum_image(fx, fy, ow, oh, blocks=shared)
        want = pool.submit(P.area_resize_blocks, img, fx, fy)
        work.append((f"{fx} x {fy} blocks, {ow} x {oh} of them", want, sums, _area(dev, img, ow, oh)))
        torch.cuda.empty_cache()
    for what, want, sums, got in work:
        _assert_same(got, want.result(), what)
        assert np.array_equal(got, (2 * sums + n) // (2 * n)), what  # round-half-up of S / n, spelled out


# ---------------------------------------------------------------------------- 4. determinism, graph replay
def test_same_bits_twice_and_from_a_graph(dev, pool):
    import torch

    from brush_amd import area_resize

    jobs = []
    for name, channels in (("chunked_256_lanes", 4), ("strip_8", 3)):
        w, h, ow, oh, want = RC.expected(name, channels)
        assert want.get("chunks") == (2, 2) or want.get("strip_rows") == 8
        img = RC.image(w, h, channels, "random", 77)
        jobs.append((torch.from_numpy(img).to(dev), (ow, oh), pool.submit(P.area_resize_integral, img, ow, oh)))
    eager = [area_resize(t, size) for t, size, _ in jobs]
    again = [area_resize(t, size) for t, size, _ in jobs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        for t, size, _ in jobs:
            area_resize(t, size)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [area_resize(t, size) for t, size, _ in jobs]
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, a, b in zip(outs, eager, again):
            assert torch.equal(o, a) and torch.equal(o, b)
    for (_, _, want), a in zip(jobs, eager):
        assert np.array_equal(a.cpu().numpy(), want.result())


# ---------------------------------------------------------------------------- 5. the nearest pick
NEAREST_SHAPES = [((16384, 2), (16383, 1)), ((16384, 1), (1, 1)), ((1, 16384), (1, 16383)), ((1030, 3), (1029, 2)),
                  ((300, 300), (257, 299))]


def _nearest(dev, d, ow, oh, offset=0):
    from brush_amd import _lib

    h, w = d.shape
    keep, src = _upload(dev, d, offset)
    out = _guarded(dev, ow * oh * d.itemsize,
                   lambda dst: _lib.lib().brush_nearest_resize(src, d.itemsize, w, h, dst, ow, oh, _stream()))
    del keep
    return out.view(np.uint16 if d.itemsize == 2 else np.uint32).reshape(oh, ow)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("src,dst", NEAREST_SHAPES)
def test_nearest_pick_at_long_sides(dev, src, dst, dtype):
    from brush_amd.dataset import resize_nearest

    (w, h), (ow, oh) = src, dst
    d = _depth_map(w, h, dtype, 3 * w + h)
    if dtype == np.float32:  # NaN payloads, both infinities and -0.0 are in the map, and have to come through as bits
        bits = d.view(np.uint32)
        bits[np.isnan(d)] |= np.random.default_rng(w).integers(1, 1 << 22, int(np.isnan(d).sum()), dtype=np.uint32)
        assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d.view(np.uint32) == 1 << 31).any()
        assert len(np.unique(bits[np.isnan(d)])) > 1
    want = _as_bits(resize_nearest(d, (oh, ow)))
    assert np.array_equal(_nearest(dev, d, ow, oh), want)


@pytest.mark.parametrize("src,dst", [((1030, 3), (1029, 2)), ((300, 300), (257, 299)), ((33, 31), (17, 16))])
def test_nearest_pick_of_a_uint16_map_at_2_mod_4(dev, src, dst):
    from brush_amd.dataset import resize_nearest

    (w, h), (ow, oh) = src, dst
    d = _depth_map(w, h, np.uint16, 11)
    keep, ptr = _upload(dev, d, 2)
    assert ptr % 4 == 2
    del keep
    assert np.array_equal(_nearest(dev, d, ow, oh, offset=2), resize_nearest(d, (oh, ow)))


# ---------------------------------------------------------------------------- 6. the accumulator switch
@pytest.mark.parametrize("strips,chunked", [("acc32_strips_of_8", "acc32_chunked"), ("acc64_strips_of_8", "acc64_chunked")])
def test_accumulator_switch_equals_the_reference(dev, pool, strips, chunked):
    """D = 16384 x 1026 and 16384 x 1027, either side of 255 D + D / 2 = 2^32.  In strips of 8 output rows: `full`, which
    takes the 32-bit accumulator to its ceiling, and a separable image a[r] b[s] (c + 1) of values up to 243, both
    against the factored reference (pyramid_ref.area_resize_separable).  One chunked row at a time over 513 or 514
    source rows: a random image against area_resize_integral."""
    import torch

    w, h, ow, oh, _ = RC.expected(strips, 3)
    cw, ch, cow, coh, _ = RC.expected(chunked, 3)
    assert (cw, ch) == (w, h)
    rng = np.random.default_rng(RC.seed_of(strips, 3))
    random = RC.image(w, h, 3, "random", RC.seed_of(chunked, 3))
    want = pool.submit(P.area_resize_integral, random, cow, coh)
    _assert_same(_area(dev, random, cow, coh), want.result(), f"{chunked} random")
    del random
    for what, a, b, g in (("full", np.full(h, 15), np.full(w, 17), np.ones(3, int)),
                          ("separable", rng.integers(0, 10, h), rng.integers(0, 10, w), np.arange(1, 4))):
        torch.cuda.empty_cache()
        img, ref = P.area_resize_separable(a, b, g, ow, oh)
        assert what != "full" or (img == 255).all()
        _assert_same(_area(dev, img, ow, oh), ref, f"{strips} {what}")
