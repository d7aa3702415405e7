"""brush_l1_ssim_loss / brush_l1_ssim_loss_gt against loss64 (tests/ref64.py), element by element: the loss value and
every v_pred element, at shapes that put the image edges on the kernels' strip (65 - WIN columns) and segment
(3 WIN + 1 rows) boundaries, one below and one past them, in the forward's (w+2) x (h+2) and the backward's w x h
tiling; tiny images; 1080p on the grid-stride L1 path and with SSIM; one 4K case.  Each test records its worst err/tol
in tests/margins.py (section loss)."""
import numpy as np
import pytest

from tests import margins
from tests import ref64 as R64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _edge_dims(m):
    """Image sizes n with n + 2 or n on the multiple m, one below it, or one past it."""
    return [m - 3, m - 2, m - 1, m, m + 1]


def _cases():
    cases = []
    i = 0
    for win in (3, 5, 7, 9, 11, 13, 15):
        ws = _edge_dims(2 * (65 - win))
        hs = _edge_dims(2 * (3 * win + 1))
        for j in range(5):
            gtc = 3 + (i % 2)
            u8 = (i // 2) % 2 == 1
            sw = (0.2, 1.0, 0.2, 0.2, 1.0)[j]
            scale = (1.0, 0.125)[(i // 3) % 2]
            content = ("random", "correlated", "blocks", "ties", "pred2")[(i + win) % 5]
            cases.append((ws[j], hs[(j + 2) % 5], win, gtc, u8, sw, scale, content))
            i += 1
    for (w, h) in ((1, 1), (1, 37), (53, 1), (2, 2)):
        for win, gtc, u8, sw, content in ((11, 3, False, 0.2, "random"), (3, 4, True, 1.0, "ties"),
                                          (15, 4, False, 0.0, "pred2")):
            cases.append((w, h, win, gtc, u8, sw, 1.0, content))
    return cases


def _inputs(w, h, gtc, u8, content, seed):
    """pred [h, w, 4] float32 in [0, 1) (in [0, 2) for "pred2": the rasterizer does not clamp), gt [h, w, gtc]."""
    rng = np.random.default_rng(seed)
    pred = rng.random((h, w, 4), dtype=np.float32)
    gt8 = rng.integers(0, 256, size=(h, w, gtc), dtype=np.uint8)
    gtf = rng.random((h, w, gtc), dtype=np.float32)
    if content == "correlated":  # half the rows follow pred
        k = h // 2
        near = np.clip(pred[:k, :, :gtc] + 0.05 * rng.standard_normal((k, w, gtc)).astype(np.float32), 0, 1)
        gt8[:k] = np.round(near * 255).astype(np.uint8)
        gtf[:k] = near
    elif content == "blocks":  # constant 13 x 13 blocks in both images: zero variance, the clamp's branch
        by, bx = np.arange(h)[:, None] // 13, np.arange(w)[None, :] // 13
        lvl = rng.integers(0, 256, size=(h // 13 + 1, w // 13 + 1, 4)).astype(np.uint8)
        gt8[:] = lvl[by, bx][..., :gtc]
        gtf[:] = R64.gt_as_f32(gt8)
        pred[:] = R64.gt_as_f32(lvl[by, bx])
        odd = ((by + bx) % 2 == 1)[..., None]
        pred[:] = np.where(odd, pred * np.float32(0.75), pred)   # every other block differs from the target
    elif content == "ties":  # exact ties: sign(0) = 0
        t = rng.random((h, w)) < 0.5
        pred[..., :gtc][t] = (R64.gt_as_f32(gt8) if u8 else gtf)[t]
    elif content == "pred2":
        pred *= np.float32(2.0)
    return pred, (gt8 if u8 else gtf)


def _run(dev, pred, gt, sw, win, scale):
    import torch

    from brush_amd.train import l1_ssim_loss

    p = torch.from_numpy(pred).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    loss, v = l1_ssim_loss(p, g, sw, win, scale)
    torch.cuda.synchronize()
    return float(loss), v.cpu().numpy()


def _check(name, loss, v, ref, enforce=True):
    w, i, bad = R64.gate(v, ref["v"], ref["tol"])
    lw = abs(loss - ref["loss"]) / ref["tol_loss"]
    if enforce:
        print(f"loss {name}: v_pred worst err/tol {w:.3f} (tol {float(ref['tol'].flat[i]):.3e} at element {i}), "
              f"loss err/tol {lw:.3f}; clamp-threshold elements priced {ref['flips']}")
        assert bad == 0, (name, w, i, bad)
        assert lw <= 1.0, (name, loss, ref["loss"], lw)
    return max(w, lw), bad + int(lw > 1.0)


def _ssim_worst(loss, v, ref):
    """Worst err/tol of the RGB elements and of the loss value, the parts the SSIM allowance (C_SSIM) prices; printed
    for the calibration factors the allowance would have at a few other values of C_SSIM."""
    grid = {}
    for c in (R64.C_SSIM, 1.0, 0.3, 0.1, 0.05):
        tol = ref["tol_fixed"][..., :3] + c * ref["tol_ssim"][..., :3]
        wv = R64.gate(v[..., :3], ref["v"][..., :3], tol)[0]
        wl = abs(loss - ref["loss"]) / (ref["tol_loss_fixed"] + c * ref["tol_loss_ssim"])
        grid[c] = (wv, wl)
    print("  SSIM calibration (C_SSIM: worst RGB err/tol, loss err/tol):",
          {c: (round(a, 4), round(b, 4)) for c, (a, b) in grid.items()})
    return grid[R64.C_SSIM]


@pytest.mark.parametrize("w,h,win,gtc,u8,sw,scale,content", _cases())
def test_loss_matches_float64(dev, w, h, win, gtc, u8, sw, scale, content):
    pred, gt = _inputs(w, h, gtc, u8, content, seed=w * 1009 + h * 7 + win)
    loss, v = _run(dev, pred, gt, sw, win, scale)
    ref = R64.loss64(pred, gt, sw, win, scale)
    worst, _ = _check(f"{w}x{h} win {win} gt {gtc}{'u8' if u8 else 'f32'} w {sw} scale {scale} {content}", loss, v, ref)
    if gtc == 3:
        assert np.all(v[..., 3] == 0.0)
    if sw > 0.0:
        margins.record("loss", "worst_ssim_rgb", _ssim_worst(loss, v, ref)[0])
    margins.record("loss", "worst", worst)
    margins.check_growth("loss", "worst", worst)


@pytest.mark.parametrize("w,h,sw,gtc,u8", [(1920, 1080, 0.0, 4, True), (1920, 1080, 0.2, 3, False),
                                           (3840, 2160, 0.2, 4, True)])
def test_loss_matches_float64_large(dev, w, h, sw, gtc, u8):
    """1080p with ssim_weight 0 runs k_l1_backward grid-stride (w h > 1024 * 256); 1080p and 4K with SSIM.  The 1080p
    SSIM case on random [0, 1] inputs also holds the allowance to its ceiling (tests/ref64.py, CEIL_LOSS): at most 1e-4
    of |v_f64| on >= 99.9 % of the elements whose v is not a cancellation of its own terms, and 1e-4 of the terms on
    >= 99.9 % of the rest."""
    pred, gt = _inputs(w, h, gtc, u8, "random", seed=w + h)
    loss, v = _run(dev, pred, gt, sw, 11, 1.0)
    ref = R64.loss64(pred, gt, sw, 11, 1.0)
    worst, _ = _check(f"{w}x{h} w {sw}", loss, v, ref)
    if sw > 0.0:
        margins.record("loss", "worst_ssim_rgb", _ssim_worst(loss, v, ref)[0])
    if sw > 0.0 and w == 1920:
        tol, av, mag = ref["tol"][..., :3], np.abs(ref["v"][..., :3]), ref["mag"][..., :3]
        canc = av < R64.CANCEL_LOSS * mag   # v a cancellation of its own terms
        frac_v = float((tol <= R64.CEIL_LOSS * av).mean())
        frac_main = float((tol[~canc] <= R64.CEIL_LOSS * av[~canc]).mean())
        frac_canc = float((tol[canc] <= R64.CEIL_LOSS * mag[canc]).mean()) if canc.any() else 1.0
        print(f"loss ceiling: tol <= {R64.CEIL_LOSS} |v| on {frac_v * 100:.3f} % of all elements (median tol/|v| "
              f"{float(np.median(tol / np.maximum(av, 1e-300))):.2e}) and on {frac_main * 100:.4f} % of those with "
              f"|v| >= {R64.CANCEL_LOSS} x its terms; the other {float(canc.mean()) * 100:.2f} %: tol <= "
              f"{R64.CEIL_LOSS} x the terms on {frac_canc * 100:.4f} %")
        margins.record("loss", "ceiling_fraction", frac_main)
        margins.record("loss", "ceiling_fraction_all", frac_v)
        assert frac_main >= R64.CEIL_LOSS_FRACTION, frac_main
        assert frac_canc >= R64.CEIL_LOSS_FRACTION, frac_canc
    margins.record("loss", "worst", worst)
    margins.check_growth("loss", "worst", worst)


def test_loss_gate_rejects_wrong_references(dev):
    """Negative controls: the GPU loss compared with a reference mutated in one way must fail the gate (padding
    WIN // 2, L1 over 3 of 4 channels, the SSIM term's sign).  The variance clamp is counted, not asserted: it can only
    act where E[a a] - mu^2 is within rounding of 0, i.e. where pred is (nearly) constant over the window, and there its
    decision cancels out of v_pred to first order.  d_mu carries -2 mu_a d_eaa (k_ssim_forward), so a change of d_eaa at
    map position j moves v_pred(p) by about g_j d_eaa_j 2 (a_p - mu_a(j)), and a_p - mu_a(j) is what the near-zero
    variance makes small (~1e-5 of the jump in the probe below).  A reference without the clamp therefore agrees with the
    kernel whatever sign the kernel's float32 variance takes; the regions below (constant blocks, and a true variance of
    ~1e-11 under the float32 rounding, at every window) print the count."""
    w, h, win = 97, 71, 11
    pred, gt = _inputs(w, h, 4, True, "blocks", seed=3)
    loss, v = _run(dev, pred, gt, 0.2, win, 1.0)
    _check("negative-control base", loss, v, R64.loss64(pred, gt, 0.2, win, 1.0))
    failed = {}
    for mut in ("pad_half", "l1_rgb", "ssim_sign"):
        _, bad = _check(mut, loss, v, R64.loss64(pred, gt, 0.2, win, 1.0, mutate=mut), enforce=False)
        failed[mut] = bad
    failed["no_clamp"] = 0
    for cw in (3, 5, 7, 9, 11, 13, 15):
        pc, gc = _inputs(64, 48, 3, False, "random", seed=cw)
        pc[8:40, 8:56] = np.float32(0.5) + np.float32(1e-5) * pc[8:40, 8:56]
        lc, vc = _run(dev, pc, gc, 0.2, cw, 1.0)
        _check(f"clamp control base win {cw}", lc, vc, R64.loss64(pc, gc, 0.2, cw, 1.0))
        failed["no_clamp"] += _check("no_clamp", lc, vc, R64.loss64(pc, gc, 0.2, cw, 1.0, mutate="no_clamp"),
                                     enforce=False)[1]
    print("loss negative controls (failing elements):", failed)
    margins.record("loss", "no_clamp_failing_elements", failed.pop("no_clamp"))
    for mut, bad in failed.items():
        assert bad > 0, mut
