"""CPU checks of the float64 references in tests/ref64.py (no GPU): adam64 against the float32 burn-form restatement,
loss64 against float64 central differences, the literal 2-D window of ssim.rs and the separable form of
tests/torch_trainer.py, and the negative-control mutations against the true references."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ref64 as R64


def _burn_f32(x, g, m, v, lr, t, lerp=None, rest=None):
    """burn 0.16 Adam::step in float32 torch, as tests/test_gpu_train.py::test_adam_step_matches_burn_form states it,
    with every constant a float32 (burn's betas are f32: 1 - beta and 1 - beta^t are float32 operations)."""
    x, g, m, v = (torch.from_numpy(np.asarray(a, np.float32)) for a in (x, g, m, v))
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    b1, b2, eps, one = f(0.9), f(0.999), f(1e-15), f(1.0)
    m = m * b1 + g * (one - b1)
    v = v * b2 + (g * g) * (one - b2)
    st = x - (m / (one - b1 ** t)) / ((v / (one - b2 ** t)).sqrt() + eps) * f(lr)
    if lerp is not None:
        r = torch.from_numpy(np.broadcast_to(rest, st.shape).copy())
        st = torch.where(r, x * (one - f(lerp)) + st * f(lerp), st)
    return st.numpy(), m.numpy(), v.numpy()


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_adam64_agrees_with_float32_burn_form(t):
    rng = np.random.default_rng(t)
    n, k = 4000, 12
    x = rng.standard_normal((n, k)).astype(np.float32)
    g = (rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-6, 1, (n, k))).astype(np.float32)
    m = (rng.standard_normal((n, k)) * 1e-2).astype(np.float32)
    v = (10.0 ** rng.uniform(-8, 0, (n, k))).astype(np.float32)
    rest = np.arange(k) >= 3
    for lerp in (None, 0.05):
        r = R64.adam64(x, g, m, v, lr=0.004, time=t, lerp=lerp, rest=rest if lerp else None)
        fx, fm, fv = _burn_f32(x, g, m, v, 0.004, t, lerp, rest)
        for got, want, tol in ((fx, r["x"], r["tol"]), (fm, r["m"], r["tol_m"]), (fv, r["v"], r["tol_v"])):
            w, i, bad = R64.gate(got, want, tol)
            assert bad == 0, (lerp, w, i)
        assert np.all(r["tol"] <= r["ceil"] * (1 + 1e-9))


def test_adam64_quaternion_chain_rule_matches_autograd():
    rng = np.random.default_rng(3)
    q = (rng.standard_normal((500, 4)) * 10.0 ** rng.uniform(-3, 3, (500, 1))).astype(np.float32)
    vq = rng.standard_normal((500, 4)).astype(np.float32)
    qt = torch.from_numpy(q).double().requires_grad_(True)
    (qt / qt.norm(dim=1, keepdim=True)).backward(torch.from_numpy(vq).double())
    g = qt.grad.numpy()
    zero = np.zeros_like(q)
    r = R64.adam64(q, vq, zero, zero, lr=0.002, time=1, quat_vjp=True)
    want = R64.adam64(q, g, zero, zero, lr=0.002, time=1)
    assert np.allclose(r["x"], want["x"], rtol=1e-12, atol=0) and np.allclose(r["m"], want["m"], rtol=1e-12, atol=0)


def test_replay64_is_k_zero_gradient_steps():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((6, 12)).astype(np.float32)
    m = (rng.standard_normal((6, 12)) * 1e-3).astype(np.float32)
    v = (10.0 ** rng.uniform(-8, -2, (6, 12))).astype(np.float32)
    rest = np.arange(12) >= 3
    t0 = np.array([20, 19, 18, 13, 12, 11])
    r = R64.replay64(x, m, v, t0, 20, lr=0.004, lerp=0.05, rest=rest)
    assert r["steps"][:, 0].tolist() == [0, 1, 2, 7, 8, 9]
    for row in range(6):
        xx, mm, vv = (a[row:row + 1].astype(np.float64) for a in (x, m, v))
        for t in range(t0[row] + 1, 21):
            s = R64.adam64(xx, np.zeros_like(xx), mm, vv, lr=0.004, time=t, lerp=0.05, rest=rest)
            xx, mm, vv = s["x"], s["m"], s["v"]
        assert np.array_equal(r["x"][row:row + 1], xx) and np.array_equal(r["m"][row:row + 1], mm)
    assert np.all(r["tol"][0] == 0.0) and np.all(r["tol"][1:] > 0.0)


def _adam_mutants():
    rng = np.random.default_rng(6)
    n = 256
    q = rng.standard_normal((n, 4)).astype(np.float32) * 3
    x = rng.standard_normal((n, 48)).astype(np.float32)
    g = rng.standard_normal((n, 48)).astype(np.float32)
    m = (rng.standard_normal((n, 48)) * 1e-2).astype(np.float32)
    v = (10.0 ** rng.uniform(-33, -1, (n, 48))).astype(np.float32)
    g[:, ::5] *= 1e-16   # v' stays near eps^2 there: where eps inside the root matters
    return q, x, g, m, v


@pytest.mark.parametrize("mutate", ["bc_tm1", "eps_in_sqrt", "lerp_coef0", "no_lerp_coef3", "abs_g", "no_quat_chain"])
def test_adam_mutations_change_the_reference(mutate):
    q, x, g, m, v = _adam_mutants()
    rest = np.arange(48) >= 3
    for t in (2, 1000):
        if mutate == "no_quat_chain":
            a = R64.adam64(q, g[:, :4], m[:, :4], v[:, :4], lr=0.002, time=t, quat_vjp=True)
            b = R64.adam64(q, g[:, :4], m[:, :4], v[:, :4], lr=0.002, time=t, quat_vjp=True, mutate=mutate)
        else:
            a = R64.adam64(x, g, m, v, lr=0.004, time=t, lerp=0.05, rest=rest)
            b = R64.adam64(x, g, m, v, lr=0.004, time=t, lerp=0.05, rest=rest, mutate=mutate)
        assert (np.abs(a["x"] - b["x"]) > a["tol"]).any(), (mutate, t)


def _pair(h, w, gtc, seed, u8=False):
    rng = np.random.default_rng(seed)
    pred = rng.random((h, w, 4), dtype=np.float32)
    gt = rng.integers(0, 256, (h, w, gtc), dtype=np.uint8) if u8 else rng.random((h, w, gtc), dtype=np.float32)
    return pred, gt


def test_loss64_blur_is_the_2d_window_of_ssim_rs():
    """The separable passes of loss64 are the 2-D window outer(g, g) with div_ceil(WIN, 2) zero padding; .t is its
    adjoint."""
    for win in (3, 11, 15):
        x = torch.rand(1, 3, 23, 41, dtype=torch.float64)
        g = torch.from_numpy(R64.window64(win))
        w2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
        want = F.conv2d(x, w2, None, padding=(win + 1) // 2, groups=3)
        blur = R64._Blur(win, (win + 1) // 2, 3)
        got = blur(x)
        assert got.shape == want.shape == (1, 3, 25, 43)
        assert float((got - want).abs().max()) <= 1e-14
        y = torch.rand_like(want)
        assert abs(float((got * y).sum()) - float((x * blur.t(y)).sum())) <= 1e-12


def test_loss64_equals_the_separable_form():
    """The value of loss64 is the L1 / SSIM combination of tests/torch_trainer.py's separable Ssim."""
    from tests.torch_trainer import Ssim

    pred, gt = _pair(37, 53, 4, 1)
    r = R64.loss64(pred, gt, 0.2, 11, 1.0, allowance=False)
    s = Ssim(11, 3, torch.device("cpu"))
    g = torch.from_numpy(R64.window64(11))
    s.wv, s.wh = g.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1), g.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1)
    p, b = torch.from_numpy(pred).double()[None], torch.from_numpy(gt).double()[None]
    ssim = s.ssim(p[..., :3], b[..., :3])
    sw = float(np.float32(0.2))   # the kernel's argument is a float32
    want = (p - b).abs().mean() * (1.0 - sw) - ssim * sw
    assert abs(r["loss"] - float(want)) <= 1e-13 * abs(float(want))


def _loss_2d(p, b, sw, win):
    """The loss as an independent float64 evaluation (literal 2-D window, one conv2d) for the central differences."""
    pt, bt = torch.from_numpy(p), torch.from_numpy(b)
    cmp = pt if b.shape[-1] == 4 else pt[..., :3]
    loss = (cmp - bt).abs().mean()
    if sw > 0:
        g = torch.from_numpy(R64.window64(win))
        w2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
        blur = lambda t: F.conv2d(t, w2, None, padding=(win + 1) // 2, groups=3)
        x, y = pt[..., :3].permute(2, 0, 1)[None], bt[..., :3].permute(2, 0, 1)[None]
        mx, my = blur(x), blur(y)
        sxx = (blur(x * x) - mx * mx).clamp_min(0)
        syy = (blur(y * y) - my * my).clamp_min(0)
        sxy = blur(x * y) - mx * my
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        ssim = (((mx * my * 2 + c1) * (sxy * 2 + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))).mean()
        loss = loss * (1.0 - sw) - ssim * sw
    return float(loss)


@pytest.mark.parametrize("w,h,win,gtc,sw", [(23, 17, 11, 4, 0.2), (9, 31, 3, 3, 1.0), (1, 7, 5, 4, 0.5)])
def test_loss64_gradient_matches_central_differences(w, h, win, gtc, sw):
    """Sampled pixels: the corners (border), the centre and a pixel one window into the image."""
    pred, gt = _pair(h, w, gtc, w + h, u8=True)
    r = R64.loss64(pred, gt, sw, win, 0.5, allowance=False)
    pts = {(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (h // 2, w // 2), (min(h - 1, win), min(w - 1, win // 2))}
    p64 = pred.astype(np.float64)
    gt64 = R64.gt_as_f32(gt).astype(np.float64)
    hstep = 1e-6
    for (y, x) in sorted(pts):
        for c in range(4):
            if c == 3 and gtc == 3:
                assert r["v"][y, x, c] == 0.0
                continue
            if abs(p64[y, x, c] - gt64[y, x, c]) < 1e-5:
                continue  # |.| is not differentiable at a tie
            a, b = p64.copy(), p64.copy()
            a[y, x, c] += hstep
            b[y, x, c] -= hstep
            fd = (_loss_2d(a, gt64, sw, win) - _loss_2d(b, gt64, sw, win)) * 0.5 / (2 * hstep)
            assert abs(fd - r["v"][y, x, c]) <= 1e-6 * max(abs(fd), 1e-3 / (h * w)), (y, x, c, fd, r["v"][y, x, c])


@pytest.mark.parametrize("mutate", ["pad_half", "no_clamp", "l1_rgb", "ssim_sign"])
def test_loss_mutations_change_the_reference(mutate):
    pred, gt = _pair(31, 29, 4, 9, u8=True)
    pred[:16, :16] = R64.gt_as_f32(gt[:1, :1])[0, 0]   # a constant block in both: the variance sits at 0
    gt[:16, :16] = gt[0, 0]
    a = R64.loss64(pred, gt, 0.2, 11, 1.0)
    b = R64.loss64(pred, gt, 0.2, 11, 1.0, mutate=mutate)
    if mutate == "no_clamp":
        # exact arithmetic never takes a variance below 0, so the clamp acts at the rounding level, on the elements
        # whose threshold the true reference prices (flips, the jump of d/d blur(a a)); a reference without the clamp
        # has no threshold to price
        assert a["flips"] > 0 and b["flips"] == 0 and np.any(b["tol"] < a["tol"])
    else:
        changed = int((np.abs(a["v"] - b["v"]) > a["tol"]).sum())
        assert changed > 0 or abs(a["loss"] - b["loss"]) > a["tol_loss"], mutate


def test_loss64_allowance_is_finite_and_prices_the_clamp():
    pred, gt = _pair(40, 40, 3, 2)
    pred[:20, :20] = 0.5
    gt[:20, :20] = 0.5
    r = R64.loss64(pred, gt, 0.2, 11, 1.0)
    assert np.all(np.isfinite(r["tol"])) and np.all(r["tol"][..., :3] > 0) and r["flips"] > 0
    assert np.all(r["tol"][..., 3] == 0.0) and np.all(r["v"][..., 3] == 0.0)
    assert math.isfinite(r["tol_loss"]) and r["tol_loss"] > 0
