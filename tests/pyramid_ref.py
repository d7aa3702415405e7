"""Host references for the device image pyramid (brush_amd/pyramid.py), independent of the kernels.

The area filter of include/brush_hip.h (brush_area_resize_u8), restated in numpy int64: x is measured in units where a
source pixel is `ow` wide and an output pixel `w` wide, so output column X covers [X w, (X+1) w), source column s covers
[s ow, (s+1) ow), the weight is their overlap, and with the same in y and D = w h

    dst[Y,X,c] = (sum_r sum_s wy[Y,r] wx[X,s] src[r,s,c] + D // 2) // D         (one rounding)

`area_resize_ref` builds the two dense weight matrices; `area_resize_blocks` is the reshape-and-sum form for sources
whose sides are multiples of an integer factor (it stays fast at large sizes); `area_resize_integral` is the same
definition for any ratio through running sums, linear in the image, sharing neither weights nor taps with the others.
The nearest-neighbour reference is brush_amd.dataset.resize_nearest.
"""
import numpy as np


def overlap_weights(n: int, on: int) -> np.ndarray:
    """[on, n] int64: row X holds the overlap of output cell [X n, (X+1) n) with every source cell [s on, (s+1) on)."""
    assert 1 <= on <= n
    X = np.arange(on, dtype=np.int64)[:, None]
    s = np.arange(n, dtype=np.int64)[None, :]
    wgt = np.maximum(0, np.minimum((X + 1) * n, (s + 1) * on) - np.maximum(X * n, s * on))
    assert (wgt.sum(axis=1) == n).all()  # every output cell is n units wide
    return wgt


def area_resize_ref(img: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """The area filter of a uint8 [h,w,c] image to [oh,ow,c], every channel on its own."""
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w, _ = img.shape
    wy, wx = overlap_weights(h, oh), overlap_weights(w, ow)
    D = np.int64(w) * np.int64(h)
    S = np.einsum("yr,rsc,xs->yxc", wy, img.astype(np.int64), wx, optimize=True)
    assert S.dtype == np.int64
    return ((S + D // 2) // D).astype(np.uint8)


MUTATIONS = ("half_down", "no_remainder", "swapped_on", "round_after_x")


def _running_sum(a: np.ndarray, axis: int, dtype) -> np.ndarray:
    """np.cumsum(a, axis, dtype).  Along axis 0 numpy walks down the columns of a C-ordered array; there the rows are
    added one after the other instead."""
    if axis != 0 or a.ndim == 1:
        return np.cumsum(a, axis=axis, dtype=dtype)
    C = np.empty(a.shape, dtype)
    C[0] = a[0]
    for r in range(1, a.shape[0]):
        np.add(C[r - 1], a[r], out=C[r], dtype=dtype, casting="unsafe")
    return C


def _cell_sums(a: np.ndarray, axis: int, on: int, edge_on: int, mutate) -> np.ndarray:
    """Along `axis` of the non-negative integer array `a` (n cells, each `on` units wide, piecewise constant): the
    integral over each of the `on` output cells [X n, (X+1) n), through F(p) = C[p // on] on + a[p // on] (p % on) with
    C the cumulative sum with a leading zero.  `edge_on` is `on` except under a mutation.  F is at most max(a) n on:
    where that stays below 2^32 everything is exact in uint32 (half the memory traffic), else it is done in int64."""
    n = a.shape[axis]
    p = np.arange(on + 1, dtype=np.int64) * n
    q, rem = p // edge_on, p % edge_on
    if mutate == "no_remainder":
        rem = rem * 0
    q = np.minimum(q, n)  # only a mutation can step past the end
    dtype = np.uint32 if int(a.max()) * n * max(on, edge_on) < 2 ** 32 else np.int64
    C = _running_sum(a, axis, dtype)
    below = np.take(C, np.maximum(q - 1, 0), axis=axis)  # C[q] of the text: the cells before cell q
    shape = [1] * a.ndim
    shape[axis] = -1
    np.moveaxis(below, axis, 0)[q == 0] = 0  # no cell lies before cell 0
    cell = np.take(a, np.minimum(q, n - 1), axis=axis).astype(dtype, copy=False)  # at p = n on the remainder is 0
    below *= dtype(edge_on)
    cell = cell * rem.astype(dtype).reshape(shape)
    below += cell  # F at every edge
    return np.diff(below, axis=axis)


def area_sums_integral(img: np.ndarray, ow: int, oh: int, mutate=None) -> np.ndarray:
    """int64 [oh,ow,c]: the weighted sums S of the definition, sum_r sum_s wy wx src, before the division by D = w h; in
    time linear in the image, with no weights and no taps: per axis, the integral of the piecewise-constant signal
    between the output cells' edges, x then y.  `mutate` (one of MUTATIONS) breaks one token for the negative
    controls of tests/test_pyramid_cpu.py."""
    assert img.dtype == np.uint8 and img.ndim == 3 and mutate in (None,) + MUTATIONS
    h, w, _ = img.shape
    assert 1 <= ow <= w and 1 <= oh <= h
    swap = mutate == "swapped_on"
    sx = _cell_sums(img, 1, ow, oh if swap else ow, mutate)  # [h, ow, c], at most 255 w
    if mutate == "round_after_x":
        sx = (sx + w // 2) // w * w
    return _cell_sums(sx, 0, oh, ow if swap else oh, mutate).astype(np.int64, copy=False)  # at most 255 w h


def area_resize_separable(a: np.ndarray, b: np.ndarray, g: np.ndarray, ow: int, oh: int):
    """(image, reference) for img[r,s,c] = a[r] b[s] g[c] (at most 255): its weighted sums factor into
    (sum_r wy a)[Y] (sum_s wx b)[X] g[c], two one-dimensional passes of `_cell_sums`, so the reference of a 16.8 M-pixel
    image costs no more than its output."""
    a, b, g = (np.asarray(v, dtype=np.int64) for v in (a, b, g))
    assert min(a.min(), b.min(), g.min()) >= 0 and a.max() * b.max() * g.max() <= 255
    a8, b8, g8 = (v.astype(np.uint8) for v in (a, b, g))  # the products fit a byte: no wrap-around
    img = a8[:, None, None] * b8[None, :, None] * g8[None, None, :]
    sy, sx = (_cell_sums(v, 0, on, on, None).astype(np.int64) for v, on in ((a, oh), (b, ow)))
    return img, round_sums(sy[:, None, None] * sx[None, :, None] * g[None, None, :], a.size * b.size)


def round_sums(S: np.ndarray, D: int, mutate=None) -> np.ndarray:
    """The definition's one rounding of the weighted sums S (overwritten): (S + D // 2) // D as uint8."""
    D = np.int64(D)
    S += (D - 1) // 2 if mutate == "half_down" else D // 2
    S //= D
    return S.astype(np.uint8)


def area_resize_integral(img: np.ndarray, ow: int, oh: int, mutate=None) -> np.ndarray:
    """The filter of `area_resize_ref` through `area_sums_integral` and the one rounding of `round_sums`."""
    return round_sums(area_sums_integral(img, ow, oh, mutate), img.shape[0] * img.shape[1], mutate)


def area_resize_blocks(img: np.ndarray, fx: int, fy: int) -> np.ndarray:
    """The same filter for w = fx ow, h = fy oh: every non-zero weight wy wx is ow oh, so S is ow oh times the sum of an
    fy x fx block, and the definition's one (S + D // 2) // D is applied to it as it stands."""
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w, c = img.shape
    assert w % fx == 0 and h % fy == 0
    ow, oh = w // fx, h // fy
    D = np.int64(w) * np.int64(h)
    S = img.reshape(oh, fy, ow, fx, c).sum(axis=(1, 3), dtype=np.int64) * (np.int64(ow) * np.int64(oh))
    return ((S + D // 2) // D).astype(np.uint8)
