"""The bucketed depth sort against numpy, element by element (pytest -m gpu).

Clouds of up to 2^20 splats sort their depth keys in three launches (depth_sort.hip, depth_sort_launch): a count and a
scatter whose digit is "bucket of key" (255 splitters from a sorted sample of S keys), then one workgroup per bucket
finishes its bucket — in LDS up to C pairs, with passes over its own range of the two global buffers above that.

Every case drives the real forward (brush_amd.render._forward_impl) on a 64 x 64 frame with the camera at the origin
looking down +z and every splat tiny on the optical axis, so every splat is visible and its depth key is the bit
pattern of mean.z.  The reference is np.argsort(z.view(np.uint32), kind="stable"): key ascending, ties by ascending
global id.  Asserted without tolerance: num_visible == n, global_from_compact_gid[:n] == the reference permutation,
and for the depth forward compact_depth[:n] == the sorted z bitwise.

The host threshold (2^20 splats, chosen from the cloud size like the sort's launch shapes) is reached here: n = 2^20
runs the bucket path and n = 2^20 + 1 the four-pass path, both against numpy.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Mirrors of brush_amd/csrc/depth_sort.hip (kSampleKeys: radix_sort.hip; kRadix, kBucketMaxN: sort_common.hpp)
S = 1024            # kSampleKeys: keys in the sample the splitters are picked from
B = 256             # kRadix: buckets
C = 8192            # kBucketLdsKeys: pairs a finish workgroup sorts in LDS
THRESHOLD = 1 << 20  # kBucketMaxN: largest cloud on the bucket path

W = H = 64
Z_MIN = np.float32(0.0100001)  # the cull keeps p_view.z > 0.01f


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True
    return torch.device("cuda:0")


def _sort_on_gpu(dev, z, deterministic=False, depth=False):
    """(num_visible, global_from_compact_gid[:n] as u32, compact_depth[:n] as u32 or None) of one forward."""
    import torch

    import brush_amd
    from brush_amd import render as R

    z = np.ascontiguousarray(z, dtype=np.float32)
    n = z.shape[0]
    means = np.zeros((n, 3), np.float32)
    means[:, 2] = z
    quats = np.zeros((n, 4), np.float32)
    quats[:, 0] = 1.0
    t = lambda a: torch.as_tensor(a, device=dev)
    cam = brush_amd.Camera([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], np.pi / 2, np.pi / 2, (0.5, 0.5))
    bufs = None
    if depth:
        bufs = (torch.empty((H, W), dtype=torch.float32, device=dev),
                torch.full((max(n, 1),), -1.0, dtype=torch.float32, device=dev))
    out, aux, u = R._forward_impl(cam, (W, H), t(means), t(np.full((n, 3), -6.0, np.float32)), t(quats),
                                  t(np.full((n, 1, 3), 0.5, np.float32)), t(np.full((n,), 2.0, np.float32)), False,
                                  None, deterministic=deterministic, expect_backward=False, depth=bufs,
                                  viewmat=np.eye(4, dtype=np.float32))
    torch.cuda.synchronize()
    perm = aux.global_from_compact_gid.cpu().numpy().view(np.uint32)[:n]
    keys = bufs[1].cpu().numpy().view(np.uint32)[:n] if depth else None
    return int(aux.num_visible.item()), perm, keys


def _check(dev, z, **kw):
    z = np.ascontiguousarray(z, dtype=np.float32)
    n = z.shape[0]
    assert n == 0 or float(z.min()) >= float(Z_MIN)
    ref = np.argsort(z.view(np.uint32), kind="stable").astype(np.uint32)
    nv, perm, keys = _sort_on_gpu(dev, z, **kw)
    assert nv == n
    np.testing.assert_array_equal(perm, ref)
    if keys is not None:
        np.testing.assert_array_equal(keys, z.view(np.uint32)[ref])


def _log_uniform(rng, n, lo=0.02, hi=500.0):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


def _float_run(start, count):
    """`count` consecutive f32 values from `start` upwards."""
    return (np.float32(start).view(np.uint32) + np.arange(count, dtype=np.uint32)).view(np.float32)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, B - 3, S - 1, S, S + 1])
def test_small_counts(dev, n):
    """Fewer keys than a wave, than buckets, than the sample: the sample is padded with the largest key, buckets are
    empty, and the order is still the reference's."""
    _check(dev, _log_uniform(np.random.default_rng(n), n))


def test_nothing_visible(dev):
    """A cloud behind the camera: the count is 0 on the device while the launches are sized for 5 splats, so the
    bucket offsets of the sort are never written and the finish kernel must not look at them."""
    nv, _, _ = _sort_on_gpu(dev, np.full(5, -1.0, np.float32))
    assert nv == 0


def test_many_tiles_many_buckets(dev):
    """20 000 keys: 20 count / scatter tiles, every bucket populated."""
    _check(dev, _log_uniform(np.random.default_rng(1), 20_000))


@pytest.mark.parametrize("n", [C, C + 1, 3 * C + 17])
def test_all_equal(dev, n):
    """One key value: one bucket (the last LDS size, then the global passes), order = ascending id."""
    _check(dev, np.full(n, 3.25, np.float32))


def test_two_narrow_clusters(dev):
    """Runs of adjacent floats at z = 1 and z = 500, each more than C keys, interleaved in id order: the splitters are
    all inside the two runs, the buckets are uneven, and their keys differ in the low bits only."""
    rng = np.random.default_rng(2)
    z = np.concatenate([_float_run(1.0, C + 500), _float_run(500.0, C + 900)])
    _check(dev, z[rng.permutation(z.shape[0])])


def test_few_distinct_values(dev):
    """7 key values, 30 000 keys: every splitter equals a key and ties run thousands long (about 4 300 per bucket)."""
    rng = np.random.default_rng(3)
    vals = np.array([0.02, 0.5, 1.0, 1.0000001, 7.0, 99.0, 500.0], np.float32)
    _check(dev, vals[rng.integers(0, 7, 30_000)])


def test_nextafter_chain(dev):
    """5 000 consecutive floats, shuffled: a splitter comparison that is off by one ulp puts a key in the wrong bucket."""
    rng = np.random.default_rng(4)
    _check(dev, _float_run(2.0 - 2500 * 2.0 ** -23, 5000)[rng.permutation(5000)])


def test_extreme_values(dev):
    """1e30, the smallest visible depth and their neighbours among ordinary keys: keys that differ in their top bits."""
    rng = np.random.default_rng(5)
    z = _log_uniform(rng, 3000)
    z[::500] = np.float32(1e30)
    z[7::500] = Z_MIN
    z[11] = np.nextafter(Z_MIN, np.float32(1.0))
    z[13] = np.nextafter(np.float32(1e30), np.float32(0.0))
    z[17] = np.float32(3.0e38)
    _check(dev, z)


@pytest.mark.parametrize("mode", ["deterministic", "depth", "deterministic_depth"])
def test_modes(dev, mode):
    """The same random cloud in deterministic mode and through the depth forward (sorted keys -> compact_depth)."""
    z = _log_uniform(np.random.default_rng(1), 20_000)
    _check(dev, z, deterministic="deterministic" in mode, depth="depth" in mode)


def test_lds_capacity_edge_depth(dev):
    """A bucket of C and one of C + 1 equal keys beside spread keys, through the depth forward: the last bucket that is
    finished in LDS and the first that is not, both with their keys written to the caller's buffer."""
    rng = np.random.default_rng(6)
    z = np.concatenate([np.full(C, 2.0, np.float32), np.full(C + 1, 40.0, np.float32), _log_uniform(rng, 4000)])
    _check(dev, z[rng.permutation(z.shape[0])], depth=True)


@pytest.mark.parametrize("n", [THRESHOLD, THRESHOLD + 1])
def test_host_threshold(dev, n):
    """The largest cloud of the bucket path (8 keys per lane in the scatter, buckets of 4096 keys on average: half of C)
    and the smallest of the four-pass path."""
    _check(dev, _log_uniform(np.random.default_rng(7), n, 1.0, 100.0), depth=True)
