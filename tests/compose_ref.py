"""Restatements of the compose kernels (include/brush_hip.h: brush_compose_forward / _backward;
brush_amd/csrc/compose.hip) in numpy: one in float32 that performs exactly the kernels' operations in their order (the
GPU tests compare bits with it), one in float64 of the same definition, with the sum of the absolute values of every
output's terms beside it (the scale a float32 evaluation's rounding bound is stated in, as tests/exposure_ref64.py).

    pred [h,w,4] premultiplied (r, g, b, alpha); gt [h,w,Cg] straight alpha, uint8 (read as b / 255) or float;
    mask [h,w] uint8 or None, a pixel is kept when there is no mask or mask != 0; background: 3 floats or None.
    With a background b (target [h,w,3]):
        t = 1 - alpha;  out.c = pred.c + t b_c;  out.w = alpha
        Cg == 4: s = 1 - G_a;  target.c = G_c G_a + s b_c          Cg == 3: target.c = G_c
    without one: out = pred, target = G ([h,w,Cg]).  A pixel that is not kept is +0 in every word of both.
    Backward, v = d L / d out:   v_pred.c = v.c;  v_pred.w = v.w - ((b_0 v_0 + b_1 v_1) + b_2 v_2)   (v.w without b);
    +0 in all four words of a pixel that is not kept.
"""
import numpy as np

F = np.float32


def gt_f32(gt):
    """The target as the kernels read it: uint8 -> (float) b / 255.0f, one correctly rounded f32 division."""
    gt = np.asarray(gt)
    if gt.dtype == np.uint8:
        return gt.astype(F) / F(255.0)
    return gt.astype(F)


def _keep(mask, shape_hw):
    return np.ones(shape_hw, dtype=bool) if mask is None else (np.asarray(mask) != 0)


def forward32(pred, gt, background=None, mask=None):
    """(out [h,w,4], target [h,w,3 | Cg]) float32, every operation one f32 operation rounded on its own."""
    assert background is not None or mask is not None
    p, g = np.asarray(pred, dtype=F), gt_f32(gt)
    cg = g.shape[2]
    if background is not None:
        b = np.asarray(background, dtype=F)
        t = F(1.0) - p[..., 3]
        out = p.copy()
        for c in range(3):
            out[..., c] = p[..., c] + t * b[c]
        target = np.empty(p.shape[:2] + (3,), dtype=F)
        if cg == 4:
            s = F(1.0) - g[..., 3]
            with np.errstate(invalid="ignore"):  # an inf or NaN under the mask is computed on, then deselected
                for c in range(3):
                    target[..., c] = g[..., c] * g[..., 3] + s * b[c]
        else:
            target[...] = g
    else:
        out, target = p.copy(), g.copy()
    if mask is not None:  # by selection: a NaN under the mask does not survive
        keep = _keep(mask, p.shape[:2])[..., None]
        out = np.where(keep, out, F(0.0))
        target = np.where(keep, target, F(0.0))
    return np.ascontiguousarray(out, dtype=F), np.ascontiguousarray(target, dtype=F)


def backward32(v_out, background=None, mask=None):
    """v_pred [h,w,4] float32 from v_out = d L / d out."""
    assert background is not None or mask is not None
    v = np.asarray(v_out, dtype=F)
    vp = v.copy()
    if background is not None:
        b = np.asarray(background, dtype=F)
        vp[..., 3] = v[..., 3] - ((b[0] * v[..., 0] + b[1] * v[..., 1]) + b[2] * v[..., 2])
    if mask is not None:
        vp = np.where(_keep(mask, v.shape[:2])[..., None], vp, F(0.0))
    return np.ascontiguousarray(vp, dtype=F)


def forward64(pred, gt, background=None, mask=None):
    """(out, target, |terms| of out, |terms| of target) in float64 from the f32 inputs (a uint8 target is b / 255 in
    float64: the kernels' f32 quotient is within 2^-24 of it, which a caller adds to its bound)."""
    p = np.asarray(pred, dtype=np.float64)
    g = np.asarray(gt).astype(np.float64) / 255.0 if np.asarray(gt).dtype == np.uint8 else np.asarray(gt, np.float64)
    cg = g.shape[2]
    if background is not None:
        b = np.asarray(background, dtype=np.float64)
        t = 1.0 - p[..., 3:4]
        out = np.concatenate([p[..., :3] + t * b, p[..., 3:4]], axis=2)
        out_mag = np.concatenate([np.abs(p[..., :3]) + (1.0 + np.abs(p[..., 3:4])) * np.abs(b), np.abs(p[..., 3:4])],
                                 axis=2)
        if cg == 4:
            a = g[..., 3:4]
            target = g[..., :3] * a + (1.0 - a) * b
            target_mag = np.abs(g[..., :3] * a) + (1.0 + np.abs(a)) * np.abs(b)
        else:
            target, target_mag = g.copy(), np.abs(g)
    else:
        out, out_mag, target, target_mag = p.copy(), np.abs(p), g.copy(), np.abs(g)
    if mask is not None:
        keep = _keep(mask, p.shape[:2])[..., None]
        out, out_mag = np.where(keep, out, 0.0), np.where(keep, out_mag, 0.0)
        target, target_mag = np.where(keep, target, 0.0), np.where(keep, target_mag, 0.0)
    return out, target, out_mag, target_mag


def backward64(v_out, background=None, mask=None):
    """(v_pred, |terms|) in float64."""
    v = np.asarray(v_out, dtype=np.float64)
    vp, mag = v.copy(), np.abs(v)
    if background is not None:
        b = np.asarray(background, dtype=np.float64)
        vp[..., 3] = v[..., 3] - v[..., :3] @ b
        mag[..., 3] = np.abs(v[..., 3]) + np.abs(v[..., :3]) @ np.abs(b)
    if mask is not None:
        keep = _keep(mask, v.shape[:2])[..., None]
        vp, mag = np.where(keep, vp, 0.0), np.where(keep, mag, 0.0)
    return vp, mag


def case(w, h, cg, gt_dtype, mask_kind, seed):
    """Deterministic inputs of one test case: (pred f32 [h,w,4], gt [h,w,cg] of gt_dtype, mask u8 [h,w] or None,
    v_out f32 [h,w,4]).  mask_kind: None, "random" (about a third zero; nonzero values vary), "zero", "full" (255).
    pred's alpha covers 0, 1 and values between; a u8 target's alpha 0 and 255."""
    rng = np.random.default_rng(seed)
    pred = rng.random((h, w, 4), dtype=F)
    flat = pred.reshape(-1, 4)
    flat[::5, 3] = 0.0
    flat[1::7, 3] = 1.0
    if gt_dtype == np.uint8:
        gt = rng.integers(0, 256, (h, w, cg), dtype=np.uint8)
        if cg == 4:
            gt.reshape(-1, 4)[::3, 3] = 255
            gt.reshape(-1, 4)[1::4, 3] = 0
    else:
        gt = rng.random((h, w, cg), dtype=F)
    if mask_kind is None:
        mask = None
    elif mask_kind == "random":
        mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
        mask[rng.random((h, w)) < 0.33] = 0
    elif mask_kind == "zero":
        mask = np.zeros((h, w), dtype=np.uint8)
    else:
        mask = np.full((h, w), 255, dtype=np.uint8)
    v_out = rng.standard_normal((h, w, 4)).astype(F)
    return pred, gt, mask, v_out
