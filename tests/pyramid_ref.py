"""Host references for the device image pyramid (brush_amd/pyramid.py), independent of the kernels.

The area filter of include/brush_hip.h (brush_area_resize_u8), restated in numpy int64: x is measured in units where a
source pixel is `ow` wide and an output pixel `w` wide, so output column X covers [X w, (X+1) w), source column s covers
[s ow, (s+1) ow), the weight is their overlap, and with the same in y and D = w h

    dst[Y,X,c] = (sum_r sum_s wy[Y,r] wx[X,s] src[r,s,c] + D // 2) // D         (one rounding)

`area_resize_ref` builds the two dense weight matrices; `area_resize_blocks` is the reshape-and-sum form for sources
whose sides are multiples of an integer factor (it stays fast at large sizes).  The nearest-neighbour reference is
brush_amd.dataset.resize_nearest.
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
