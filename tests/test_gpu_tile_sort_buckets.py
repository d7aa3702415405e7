"""The bucketed tile sort against the CPU oracle, element by element (pytest -m gpu).

Frames of 257 to 65 535 tiles sort their (tile id, compact gid) pairs in three launches in the default mode
(tile_sort.hip, tile_sort_launch): a count and a scatter on the top 8 of the id's `sig` significant bits, then one
workgroup per bucket orders its bucket by the `sig - 8` bits below in chunks of C pairs and stores the bin edges of its
tiles.  Every other frame, the deterministic mode and every intersection capacity above 512 x 16 384 keep the LSD
passes.

Every case drives the real forward (brush_amd.render._forward_impl, DEBUG_POISON on) in the default mode and compares
every integer output with the oracle's, without tolerance and without skipped elements
(tests.binning_check.assert_integer_parity: counts, compact_gid_from_isect[:I], every word of tile_bins), then runs
assert_binning_properties (bins partition [0, I) in tile order, compact gids strictly ascending inside a bin: the
stability of the finish pass).  Each case also states which path it takes (`uses_buckets`, the host's rule restated) and
asserts the shape it names (occupied tiles, I, the scatter's keys per lane) on the oracle's outputs.

`pixel_cloud` puts one tiny splat (a 2-pixel radius) at the centre of a chosen tile, so a case chooses its occupied
tiles exactly; depths are distinct and shuffled, so the compact (depth) order differs from the input order.  The whole
module, oracle included, takes 3.4 s on one MI355X; the largest case (2.2 M entries) about half a second.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import binning_clouds as BC
from tests import test_gpu_render as RT

pytestmark = pytest.mark.gpu

# Mirrors of brush_amd/csrc/tile_sort.hip (kTileFinishChunk) and sort_common.hpp (the rest)
B = 256                     # kRadix: buckets
C = 8192                    # kTileFinishChunk: pairs a finish workgroup ranks at a time (its only internal switch)
SORT_THREADS = 1024         # kSortThreads
TARGET_TILES = 128          # kSortTargetTiles
FUSED_MAX = 512 * 16384     # sort_is_fused: largest capacity of the two-launch pass shape


def sig_bits(num_tiles):
    return (num_tiles - 1).bit_length()


def uses_buckets(cap, num_tiles, deterministic=False):
    """tile_sort_launch's rule, as render_forward_impl calls it."""
    return (not deterministic) and cap <= FUSED_MAX and 8 < sig_bits(num_tiles) <= 16 and num_tiles.bit_length() <= 16


def sort_items(n):
    """Keys per lane of the count / scatter pair for n keys."""
    k = 1
    while k < 16 and SORT_THREADS * k * TARGET_TILES < n:
        k *= 2
    return k


def pixel_cloud(w, h, tiles, seed, depth_order=None):
    """One tiny splat at the centre of tile tiles[i] (row-major tile index) for every i.  depth_order[i] (default: a
    random permutation) is the rank of splat i by depth, i.e. its compact gid."""
    tiles = np.asarray(tiles, np.int64)
    n = tiles.shape[0]
    tbx = (w + 15) // 16
    rng = np.random.default_rng(seed)
    order = rng.permutation(n) if depth_order is None else np.asarray(depth_order)
    d = 6.0 + 4.0 * (order.astype(np.float64) + 0.5) / max(n, 1)  # distinct in f32 up to millions of splats
    focal = 0.5 * w
    px, py = (tiles % tbx) * 16.0 + 8.0, (tiles // tbx) * 16.0 + 8.0
    means = np.stack([(px - 0.5 * w) * d / focal, (py - 0.5 * h) * d / focal, d - 8.0], axis=1)
    quats = np.zeros((n, 4))
    quats[:, 0] = 1.0
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    return dict(means=f32(means), log_scales=f32(np.repeat(np.log(0.05 * d / focal)[:, None], 3, axis=1)),
                quats=f32(quats), sh=f32(rng.uniform(-1.0, 1.0, (n, 1, 3))), raw_opac=f32(np.full(n, -1.0)))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True
    return torch.device("cuda:0")


def _gpu(dev, cloud, w, h, cap=None, deterministic=False):
    import torch

    from brush_amd import render as R

    p = {k: RT._t(v, dev) for k, v in cloud.items()}
    _, aux, _ = R._forward_impl(RT._camera(w, h), (w, h), p["means"], p["log_scales"], p["quats"], p["sh"],
                                p["raw_opac"], False, cap, deterministic=deterministic, expect_backward=False)
    torch.cuda.synchronize()
    assert aux.deterministic == deterministic
    u = R.uniforms_to_numpy(aux)
    return BK.aux_arrays(aux, u["num_visible"]), u, int(aux.max_intersects)


def _check(dev, cloud, w, h, cap=None, buckets=True):
    """Default mode against the oracle.  Returns (got, oracle aux, occupied tile indices, I)."""
    got, u, cap = _gpu(dev, cloud, w, h, cap)
    num_tiles = int(u["tile_bounds"][0]) * int(u["tile_bounds"][1])
    assert uses_buckets(cap, num_tiles) == buckets, (cap, num_tiles)
    _, oa = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"], cloud["raw_opac"],
                             max_intersects=cap)
    V, I = BK.assert_integer_parity(got, oa)
    BK.assert_binning_properties(got)
    bins = oa["tile_bins"].reshape(-1, 2).astype(np.int64)
    occupied = np.flatnonzero(bins[:, 1] > bins[:, 0])
    print(f"[tile sort] {w}x{h} tiles {num_tiles} sig {sig_bits(num_tiles)} cap {cap} V {V} I {I} occupied "
          f"{occupied.size} overflow {got['overflow']} buckets {buckets}")
    return got, oa, occupied, I


SMALL = dict(seed=23, fr_mid=0.1, fr_big=0.05, fr_thin=0.02)


@pytest.mark.parametrize("w,h,tiles,n,buckets", [
    (256, 256, 256, 3000, False),      # 8 bits: the one-pass path
    (272, 272, 289, 3000, True),       # 9 bits: shift 1, two tiles per bucket, buckets 145 .. 255 empty
    (400, 400, 625, 3000, True),       # 10 bits, the last bucket holds tile 624 alone
    (4096, 4080, 65280, 2000, True),   # 16 bits, shift 8: 256 tiles per bucket
    (4112, 4096, 65792, 2000, False),  # 17 bits: the three-pass path
])
def test_path_switch_on_tile_count(dev, w, h, tiles, n, buckets):
    """Either side of both ends of the tile-count range, and inside it."""
    got, oa, occupied, I = _check(dev, BC.directed_cloud(n, w, h, **SMALL), w, h, buckets=buckets)
    assert got["tile_bins"].shape[0] * got["tile_bins"].shape[1] == tiles and I > n and not got["overflow"]


def test_capacity_above_the_fused_shape_keeps_the_passes(dev):
    """The same 625-tile frame with a capacity above 512 x 16 384: the three-launch pass shape, not the buckets."""
    _check(dev, BC.directed_cloud(3000, 400, 400, **SMALL), 400, 400, cap=FUSED_MAX + 1, buckets=False)


@pytest.mark.parametrize("n", [1, 3, 63, 200])
def test_few_entries(dev, n):
    """Fewer entries than a wave and than buckets, on random tiles of a 4096-tile frame."""
    rng = np.random.default_rng(n)
    tiles = rng.integers(0, 4096, n)
    _, _, occupied, I = _check(dev, pixel_cloud(1024, 1024, tiles, seed=n), 1024, 1024)
    assert I == n and np.array_equal(occupied, np.unique(tiles))


# 1024 x 1024: 4096 tiles, 12 bits, 16 tiles per bucket, every bucket exists.
_BUCKET_CONTENTS = {
    "one_tile_per_bucket": np.arange(256) * 16 + 5,
    "every_tile": np.arange(4096),
    "both_ends_middle_empty": np.concatenate([np.arange(256) * 16, np.arange(256) * 16 + 15]),
    "first_and_last_bucket_only": np.concatenate([np.arange(16), 4080 + np.arange(16)]),
}


@pytest.mark.parametrize("name", list(_BUCKET_CONTENTS))
def test_bucket_contents(dev, name):
    """Three splats on each chosen tile, shuffled: which sub-digits of a bucket are present decides which edges are
    stored and where the runs start."""
    want = _BUCKET_CONTENTS[name]
    tiles = np.random.default_rng(5).permutation(np.repeat(want, 3))
    _, _, occupied, I = _check(dev, pixel_cloud(1024, 1024, tiles, seed=6), 1024, 1024)
    assert I == 3 * want.size and np.array_equal(occupied, np.sort(want))


@pytest.mark.parametrize("w,h", [(272, 272), (400, 400)])
def test_last_bucket_partly_beyond_the_frame(dev, w, h):
    """289 tiles (bucket 144 = tiles 288, 289: one exists) and 625 tiles (bucket 156 = tiles 624 .. 627: one exists),
    every tile occupied twice."""
    num_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    tiles = np.random.default_rng(7).permutation(np.repeat(np.arange(num_tiles), 2))
    _, _, occupied, I = _check(dev, pixel_cloud(w, h, tiles, seed=8), w, h)
    assert I == 2 * num_tiles and occupied.size == num_tiles


@pytest.mark.parametrize("n", [C - 1, C, C + 1, 3 * C + 17])
def test_one_tile_holds_everything(dev, n):
    """n tiny splats on one pixel of a 289-tile frame: one bucket, one tile, on either side of the finish kernel's chunk
    size and over several chunks (the digit totals are then counted in a pass of their own)."""
    _, oa, occupied, I = _check(dev, pixel_cloud(272, 272, np.full(n, 3 * 17 + 4), seed=n), 272, 272)
    assert I == n and occupied.tolist() == [3 * 17 + 4]


@pytest.mark.parametrize("n", [C - 1, C, C + 1, 3 * C + 17])
def test_two_tiles_of_one_bucket_interleaved(dev, n):
    """The same counts on tiles 54 and 55 (bucket 27 of the 289-tile frame), alternating in compact gid order: every
    wave's piece of every chunk holds both digits, and a rank that is not in index order breaks the strictly ascending
    gids inside a bin."""
    tiles = 54 + (np.arange(n) & 1)
    got, oa, occupied, I = _check(dev, pixel_cloud(272, 272, tiles, seed=n, depth_order=np.arange(n)), 272, 272)
    assert I == n and occupied.tolist() == [54, 55]
    assert np.array_equal(got["compact_gid_from_isect"][:n],
                          np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)]).astype(np.uint32))


def test_large_splats_span_many_buckets(dev):
    """Splats of hundreds of tiles each (the emitter's walk queue): every splat's entries land in many buckets."""
    cloud = BC.directed_cloud(2500, 1024, 1024, seed=29, fr_mid=0.1, fr_big=0.7, fr_thin=0.1, big_sigma=(40, 90))
    got, oa, occupied, I = _check(dev, cloud, 1024, 1024)
    V = int(oa["num_visible"][0])
    assert I > 150 * V and occupied.size > 4000


def test_nothing_visible(dev):
    """A cloud behind the camera on a 625-tile frame: I = 0 on the device with launches sized for the capacity; no
    scatter workgroup runs, the bucket offsets are leftovers of the previous forward and no bin is written."""
    _check(dev, BC.directed_cloud(3000, 400, 400, **SMALL), 400, 400)  # leaves offsets behind
    cloud = BC.directed_cloud(500, 400, 400, n_hidden=500, **SMALL)
    got, oa, occupied, I = _check(dev, cloud, 400, 400, cap=20_000)
    assert I == 0 and occupied.size == 0 and not got["tile_bins"].any()


@pytest.mark.parametrize("cap", [1, 1023, 1025, 9000])
def test_truncated_list(dev, cap):
    """max_intersects below the scene's intersection count on a 625-tile frame: overflow is flagged, I is the capacity
    and the truncated list and its bins are the oracle's with the same capacity."""
    got, oa, occupied, I = _check(dev, BC.directed_cloud(3000, 400, 400, **SMALL), 400, 400, cap=cap)
    assert got["overflow"] == 1 and I == cap and int(oa["cum_tiles_hit"][-1]) > 2 * 9000


def test_modes_agree(dev):
    """One multi-bucket scene in the deterministic mode (the LSD passes and k_tile_bin_edges) and in the default mode
    (the buckets): identical compact_gid_from_isect[:I] and tile_bins."""
    cloud = BC.directed_cloud(20_000, 1024, 1024, **SMALL)
    a, u, cap = _gpu(dev, cloud, 1024, 1024, deterministic=False)
    b, _, _ = _gpu(dev, cloud, 1024, 1024, deterministic=True)
    assert uses_buckets(cap, 4096) and not uses_buckets(cap, 4096, deterministic=True)
    I = a["num_intersections"]
    assert I == b["num_intersections"] and I > 100_000
    assert np.array_equal(a["compact_gid_from_isect"][:I], b["compact_gid_from_isect"][:I])
    assert np.array_equal(a["tile_bins"], b["tile_bins"])
    BK.assert_binning_properties(a)


def test_sixteen_keys_per_lane(dev):
    """150 000 splats with mid-size footprints on 1920 x 1080 (8160 tiles): more than 2^20 entries, so the count and
    scatter kernels take 16 keys per lane, which the depth sort's bucket scatter never does.  Against the oracle."""
    cloud = BC.directed_cloud(150_000, 1920, 1080, seed=31, fr_mid=0.25, fr_big=0.02, fr_thin=0.01)
    got, oa, occupied, I = _check(dev, cloud, 1920, 1080)
    assert sort_items(I) == 16 and I <= FUSED_MAX and not got["overflow"]
