"""The MCMC strategy on the GPU: the three kernels against the float64 restatement of tests/mcmc_ref64.py, the trainer's
strategy="mcmc" path, and a scene trained end to end under a splat budget.

The worst figures every gate met are written to profiles/mcmc_margins.json (as profiles/pose_margins.json is for the
pose gates)."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mcmc_ref64 as M
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
COUNTS = [0, 1, 63, 64, 65, 257, 1000]
MARGINS = {}

# The generator gate.  Worst |xi_gpu - xi_ref| / max(1, |xi_ref|) against the float64 restatement over n = 1000 x 4
# steps (seed 42, steps 0..3), measured on the MI355X: f32 log / sin / cos and one rounding of 2 pi u.  The gate is 8 x
# that worst value (the factor covers other draws), and never looser than 1e-4.
XI_WORST_MEASURED = 1.6584e-06
XI_GATE = min(8.0 * XI_WORST_MEASURED, 1e-4)

# The arithmetic gate of the noise: |delta_gpu - delta_ref| <= K U sum|terms| + U |mean|.  K counts the roundings (unit
# roundoff U each; expf budgeted at 2 ulp = 4 U) on the deepest path of the kernel's expression tree:
#   gate   1 - o = 1 / (1 + expf(raw)): 6;  minus 0.995f: absolute 8 U;  times -100: absolute 900 U, which is the relative
#          error of the expf behind it; expf, 1 +, 1 /: 906;  times scale, times xi: 908
#   R      s2 4, sqrt 3, 1 / 4, q inv 5, products 11, sum 12, 1 - 2 (..) 13
#   t = (R^T w) exp(2 s):  13 + 908 + 1 (product) + 2 (sums) = 924;  expf 4, product 1: 929
#   R t:   13 + 929 + 1 + 2 = 945
# so K = 945, all but 39 of it the factor 100 inside the gate's exponential; the final `mean + delta` is the U |mean| term.
K_NOISE = 945.0


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    if MARGINS:
        path = os.environ.get("BRUSH_MCMC_MARGINS") or os.path.join(ROOT, "profiles", "mcmc_margins.json")
        try:
            old = {}
            if os.path.exists(path):
                with open(path) as f:
                    old = json.load(f)
            old.update(MARGINS)
            with open(path, "w") as f:
                json.dump(old, f, indent=1, sort_keys=True)
        except (OSError, ValueError) as e:  # a read-only checkout: never turn a finished run red from here
            print(f"mcmc margins not written: {e!r}")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


def _worse(name, value):
    MARGINS[name] = max(float(value), MARGINS.get(name, 0.0))


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _cloud(n, seed=0):
    """Every fourth splat opaque (o = 0.8, gate ~ e^-79), faint (o = 0.001, gate ~ 0.6), anisotropic (scales 100 x
    apart) or with an un-normalised rotation; the rest of each splat random."""
    rng = np.random.default_rng(seed + n)
    means = rng.uniform(-2.0, 2.0, (n, 3))
    ls = np.log(rng.uniform(0.01, 0.2, (n, 3)))
    rot = rng.normal(size=(n, 4))
    rot /= np.maximum(np.linalg.norm(rot, axis=1, keepdims=True), 1e-9)
    o = rng.uniform(0.0005, 0.02, n)  # where the gate is neither 0 nor 1
    kind = np.arange(n) % 4
    o[kind == 0] = 0.8
    o[kind == 1] = 0.001
    ls[kind == 2] = np.log(0.002) + np.log(np.array([1.0, 10.0, 100.0]))
    rot[kind == 3] *= rng.uniform(0.2, 5.0, (int((kind == 3).sum()), 1))
    raw = np.log(o / (1.0 - o))
    return [np.ascontiguousarray(a, dtype=np.float32) for a in (means, ls, rot, raw)]


def _noise(dev, arrays, scale, seed, step, want_xi=True):
    """brush_mcmc_inject_noise on copies of the arrays: (means after, xi or None), the inputs checked unchanged."""
    import torch

    from brush_amd import mcmc

    t = [torch.from_numpy(a).to(dev) for a in arrays]
    n = arrays[0].shape[0]
    xi = torch.full((n, 3), float("nan"), device=dev) if want_xi else None
    mcmc.inject_noise(t[0], t[1], t[2], t[3], n, scale, seed, step, _stream(), xi_out=xi)
    torch.cuda.synchronize()
    for a, b in zip(arrays[1:], t[1:]):
        assert _np(b).tobytes() == a.tobytes()
    return _np(t[0]), (None if xi is None else _np(xi))


def _xi_err(xi, ref):
    return float((np.abs(xi.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()) if xi.size else 0.0


# ---------------------------------------------------------------------------- 1. noise: the generator
@pytest.mark.parametrize("n", COUNTS)
def test_noise_generator_matches_philox_restatement(dev, n):
    arrays = _cloud(n)
    for seed, step in ((42, 0), (0xFEDCBA9876543210, 7), (1 << 32, 0xFFFFFFFF)):
        _, xi = _noise(dev, arrays, 80.0, seed, step)
        assert xi.shape == (n, 3) and np.isfinite(xi).all()
        err = _xi_err(xi, M.xi64(seed, step, n))
        print(f"xi n={n} seed={seed:#x} step={step}: worst {err:.3e} (gate {XI_GATE:.3e})")
        assert err <= XI_GATE


def test_noise_generator_margin_repeatability_and_moments(dev):
    arrays = _cloud(1000)
    worst, xis = 0.0, []
    for step in range(4):
        _, xi = _noise(dev, arrays, 80.0, 42, step)
        worst = max(worst, _xi_err(xi, M.xi64(42, step, 1000)))
        xis.append(xi)
    print(f"xi worst over 1000 x 4: {worst:.4e}, gate {XI_GATE:.4e}")
    MARGINS["xi_worst"], MARGINS["xi_gate"] = worst, XI_GATE
    assert worst <= XI_GATE
    # a step is a pure function of (seed, step, g): the same bits again, and for another n
    m2, xi2 = _noise(dev, arrays, 80.0, 42, 1)
    m3, _ = _noise(dev, arrays, 80.0, 42, 1, want_xi=False)
    assert xi2.tobytes() == xis[1].tobytes() and m2.tobytes() == m3.tobytes()
    small = [a[:65].copy() for a in arrays]
    m65, xi65 = _noise(dev, small, 80.0, 42, 1)
    assert xi65.tobytes() == xis[1][:65].tobytes() and m65.tobytes() == m2[:65].tobytes()
    # another step or seed: other draws
    assert (xis[0] != xis[1]).mean() > 0.99
    _, other = _noise(dev, arrays, 80.0, 43, 1)
    _, high = _noise(dev, arrays, 80.0, 42 + (1 << 32), 1)
    assert (other != xis[1]).mean() > 0.99 and (high != xis[1]).mean() > 0.99
    # 3000 values: mean and variance within 5 sigma of 0 and 1
    v = xis[0].astype(np.float64).ravel()
    assert v.size == 3000 and abs(v.mean()) <= 5.0 / math.sqrt(3000) and abs(v.var() - 1.0) <= 5.0 * math.sqrt(2.0 / 3000)


# ---------------------------------------------------------------------------- 2. noise: the arithmetic
@pytest.mark.parametrize("n", COUNTS)
def test_noise_arithmetic_against_ref64(dev, n):
    arrays = _cloud(n, seed=1)
    scale = 5e5 * 1.6e-4
    after, xi = _noise(dev, arrays, scale, 7, 3)
    if n == 0:
        return
    scale32 = float(np.float32(scale))
    delta, terms = M.noise_delta64(arrays[1], arrays[2], arrays[3], xi, scale32)
    got = after.astype(np.float64) - arrays[0].astype(np.float64)
    bound = K_NOISE * U * terms + U * np.abs(after.astype(np.float64))
    ratio = float((np.abs(got - delta) / bound).max())
    print(f"noise arithmetic n={n}: worst err/bound {ratio:.4f}")
    _worse("noise_arithmetic_worst_ratio", ratio)
    assert ratio <= 1.0
    if n >= 64:
        moved = np.abs(got).max(1)
        kind = np.arange(n) % 4
        assert (moved[kind == 0] == 0).all()          # opaque: the gate shuts the noise off
        assert (moved[kind == 1] > 0).mean() > 0.9    # faint: it moves
        gate = M.gate64(arrays[3])
        assert gate[kind == 0].max() < 1e-30 and 0.5 < gate[kind == 1].min() < 0.7


def test_noise_scale_zero_leaves_the_means(dev):
    arrays = _cloud(257, seed=2)
    after, _ = _noise(dev, arrays, 0.0, 7, 3)
    assert np.array_equal(after, arrays[0])


# ---------------------------------------------------------------------------- 3. regulariser
def _reg(dev, n, opacity_reg, scale_reg, seed=0):
    import torch

    from brush_amd import mcmc

    rng = np.random.default_rng(100 + n + seed)
    raw = rng.normal(0.0, 3.0, n).astype(np.float32)
    ls = np.log(rng.uniform(0.005, 2.0, (n, 3))).astype(np.float32)
    v_opac = (rng.normal(size=n) * 1e-4).astype(np.float32)
    v_scales = (rng.normal(size=(n, 3)) * 1e-4).astype(np.float32)
    if n > 2:
        v_opac[0], v_opac[1], v_scales[0, 0], v_scales[1, 2] = 0.0, -0.0, -0.0, 0.0
    t = [torch.from_numpy(a).to(dev) for a in (raw, ls, v_opac, v_scales)]
    mcmc.reg_grads(t[0], t[1], n, opacity_reg, scale_reg, t[2], t[3], _stream())
    torch.cuda.synchronize()
    assert _np(t[0]).tobytes() == raw.tobytes() and _np(t[1]).tobytes() == ls.tobytes()
    return raw, ls, v_opac, v_scales, _np(t[2]), _np(t[3])


@pytest.mark.parametrize("n", COUNTS)
def test_regulariser_gradients_against_ref64(dev, n):
    for reg_o, reg_s in ((0.01, 0.01), (0.5, 0.0), (0.0, 3.0)):
        raw, ls, v_o, v_s, got_o, got_s = _reg(dev, n, reg_o, reg_s)
        if n == 0:
            continue
        t_o, t_s = M.reg_terms64(raw, ls, float(np.float32(reg_o)), float(np.float32(reg_s)))
        for name, before, term, got in (("opac", v_o, t_o, got_o), ("scales", v_s, t_s, got_s)):
            before = before.astype(np.float64)
            bound = 4.0 * U * (np.abs(before) + np.abs(term))
            err = np.abs(got.astype(np.float64) - (before + term))
            assert (err <= bound).all(), (name, n, float((err / np.maximum(bound, 1e-300)).max()))
            if bound.max() > 0:
                _worse("regulariser_worst_ratio", (err[bound > 0] / bound[bound > 0]).max())
        if reg_s == 0.0:
            assert got_s.tobytes() == v_s.tobytes()
        if reg_o == 0.0:
            assert got_o.tobytes() == v_o.tobytes()
    raw, ls, v_o, v_s, got_o, got_s = _reg(dev, n, 0.0, 0.0)
    assert got_o.tobytes() == v_o.tobytes() and got_s.tobytes() == v_s.tobytes()  # -0.0 included


def test_regulariser_terms_are_the_autograd_gradients():
    import torch

    rng = np.random.default_rng(4)
    raw, ls = rng.normal(0.0, 3.0, 65), np.log(rng.uniform(0.005, 2.0, (65, 3)))
    a, b = torch.tensor(raw, dtype=torch.float64, requires_grad=True), torch.tensor(ls, dtype=torch.float64,
                                                                                    requires_grad=True)
    (0.01 * torch.sigmoid(a).mean() + 0.02 * torch.exp(b).mean()).backward()
    t_o, t_s = M.reg_terms64(raw, ls, 0.01, 0.02)
    assert np.allclose(a.grad.numpy(), t_o, rtol=1e-13, atol=0) and np.allclose(b.grad.numpy(), t_s, rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------- 4. relocation
def _ulps(a, b):
    """Distance in f32 units in the last place between two f32 arrays (ordered-integer view)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _relocation_rows(m):
    o = np.array([0.3]) if m == 1 else np.geomspace(0.005, 1.0 - 1e-7, m)
    if m >= 65:  # the far end needs more than a log-spaced grid puts there
        o[-16:] = 1.0 - np.geomspace(1e-2, 1e-7, 16)
    ratios = np.array([(7 * g) % 52 + 1 for g in range(m)], np.int64)  # 1..52, every value once m >= 52
    ratios[ratios == 52] = 60
    rng = np.random.default_rng(m)
    raw = np.log(o / (1.0 - o)).astype(np.float32)
    ls = np.log(rng.uniform(0.002, 1.0, (m, 3))).astype(np.float32)
    return raw, ls, ratios


@pytest.mark.parametrize("m", [0, 1, 65, 1000])
def test_relocation_against_ref64(dev, m):
    import torch

    from brush_amd.mcmc import relocation

    raw, ls, ratios = _relocation_rows(m)
    min_opacity = 0.005
    for rt in (ratios, np.ones_like(ratios)):
        t = [torch.from_numpy(a).to(dev) for a in (raw, ls, rt)]
        new_raw, new_ls = relocation(t[0], t[1], t[2], min_opacity)
        torch.cuda.synchronize()
        assert _np(t[0]).tobytes() == raw.tobytes() and _np(t[1]).tobytes() == ls.tobytes()
        assert _np(t[2]).tobytes() == rt.tobytes() and tuple(new_raw.shape) == (m,) and tuple(new_ls.shape) == (m, 3)
        if m == 0:
            continue
        want_raw, want_ls = M.relocation_rows64(raw, ls, rt, float(np.float32(min_opacity)))
        d_raw, d_ls = _ulps(_np(new_raw), want_raw.astype(np.float32)), _ulps(_np(new_ls), want_ls.astype(np.float32))
        print(f"relocation m={m}: worst ulps raw {int(d_raw.max())} log_scales {int(d_ls.max())}")
        _worse("relocation_worst_ulps", max(d_raw.max(), d_ls.max()))
        assert d_raw.max() <= 2 and d_ls.max() <= 2
        if rt is not ratios:  # one copy: the row comes back as it went in, wherever the clamp does not act
            o = M.sigmoid(raw)
            free = (o >= float(np.float32(min_opacity))) & (o <= 1.0 - 2.0 ** -24)
            assert free.sum() >= m - 2
            assert _ulps(_np(new_ls), ls).max() <= 1 and _ulps(_np(new_raw)[free], raw[free]).max() <= 2
    if m >= 65:
        assert set(range(1, 52)) | {60} <= set(int(r) for r in ratios)


# ---------------------------------------------------------------------------- 5. trainer
PARAMS = ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")


def _views(dev, w=96, h=80):
    import torch

    cams = [c for _, c in TL._ring_cameras(4, w, h)]
    gts = [torch.from_numpy(TL.E.noise_image(w, h, 3 + (i % 2), 50 + i)).to(dev) for i in range(4)]
    return cams, gts


def _splats(dev, n=1000, faint=50):
    import torch

    from brush_amd import Splats

    s = Splats.from_random_config(n, 3, (np.full(3, -1.0), np.full(3, 1.0)), np.random.default_rng(3), dev)
    with torch.no_grad():
        s.raw_opacity[:faint] = math.log(0.001 / 0.999)
    return s


def _bits(splats, tr):
    return tuple(_np(getattr(splats, k)).tobytes() for k in PARAMS) + (_np(tr.moment1).tobytes(),
                                                                         _np(tr.moment2).tobytes())


def _mcmc_cfg(**kw):
    from brush_amd import TrainConfig

    return TrainConfig(**{**dict(strategy="mcmc", warmup_steps=5, refine_every=10, mcmc_cap_max=1100), **kw})


def test_trainer_relocates_grows_and_keeps_the_optimizer(dev, monkeypatch):
    import torch

    from brush_amd import SplatTrainer, mcmc

    cams, gts = _views(dev)
    splats = _splats(dev)
    tr = SplatTrainer(splats, _mcmc_cfg())
    seen = {}
    real_refine, real_split = mcmc.refine, mcmc._split

    def split(params, idx, min_opacity):
        dead = torch.nonzero(torch.sigmoid(params["raw_opacity"]) <= min_opacity).squeeze(1)
        seen["calls"].append((idx.clone(), dead.clone()))
        return real_split(params, idx, min_opacity)

    def refine(trainer, s):
        seen.update(calls=[], n=s.num_splats(), m1=trainer.moment1.clone(), m2=trainer.moment2.clone())
        return real_refine(trainer, s)

    monkeypatch.setattr(mcmc, "_split", split)
    monkeypatch.setattr(mcmc, "refine", refine)
    counts, refined_at = [], []
    for i in range(32):
        it = tr.iter
        tr.step(splats, cams[i % 4], gts[i % 4], 1.0)
        counts.append(splats.num_splats())
        assert splats.num_splats() <= 1100
        if tr.last_refine is None:
            continue
        refined_at.append(it)
        st = tr.last_refine
        assert isinstance(st, mcmc.McmcRefineStats)
        n_old, n_new, ncoef = seen["n"], splats.num_splats(), int(splats.sh_coeffs.shape[1])
        assert n_new == n_old + st.num_added
        if len(refined_at) == 1:
            assert st.num_relocated > 0 and len(seen["calls"]) == 2
        touched = torch.zeros(n_new, dtype=torch.bool, device=dev)
        touched[n_old:] = True
        for idx, _ in seen["calls"]:
            touched[idx] = True
        if st.num_relocated > 0:
            dead = seen["calls"][0][1]
            assert dead.numel() == st.num_relocated
            touched[dead] = True
            # a relocated splat is a copy of the row it was drawn onto (the growth behind it rewrites opacity and
            # scale of the rows it samples, never these three)
            src = seen["calls"][0][0]
            for k in ("means", "rotation", "sh_coeffs"):
                assert torch.equal(getattr(splats, k).detach()[dead], getattr(splats, k).detach()[src])
        keep = torch.nonzero(~touched).squeeze(1)
        assert 0 < keep.numel() <= n_old and (keep.numel() < n_old) == (st.num_relocated + st.num_added > 0)
        for before, after in ((seen["m1"], tr.moment1), (seen["m2"], tr.moment2)):
            assert after.numel() == n_new * (11 + 3 * ncoef)
            for old, new in zip(mcmc.moment_segments(before, n_old, ncoef), mcmc.moment_segments(after, n_new, ncoef)):
                assert torch.equal(old[keep].view(torch.int32), new[keep].view(torch.int32))
                assert bool((new[touched] == 0).all()) and bool(old[keep].abs().sum() > 0)
        assert splats.xys_dummy.shape[0] == n_new
    # the trigger (iter % refine_every == 1 past the warmup) fires at 11 and 21, and again in the last of the 32 steps,
    # where the count sits at the cap and nothing is added
    assert refined_at == [11, 21, 31] and tr.last_refine.num_added == 0
    assert counts[10] == 1000 and counts[11] == 1050 and counts[20] == 1050 and counts[21] == 1100 and counts[-1] == 1100
    assert tr.opt_time == 32 and tr.iter == 32
    for k in PARAMS:
        assert bool(torch.isfinite(getattr(splats, k)).all()), k
    assert bool(torch.isfinite(tr.moment1).all()) and bool(torch.isfinite(tr.moment2).all())
    assert tr._lazy is None  # the deferred-SH state is never created


def _run(dev, cfg, steps, fused=None):
    import torch

    from brush_amd import SplatTrainer

    cams, gts = _views(dev)
    splats = _splats(dev)
    tr = SplatTrainer(splats, cfg)
    if fused is not None:
        tr.fused_backward = fused
    out = []
    for i in range(steps):
        tr.step(splats, cams[i % 4], gts[i % 4], 1.0)
        out.append(_bits(splats, tr))
    tr.sync(splats)
    torch.cuda.synchronize()
    return out, splats, tr


def test_zero_regulariser_is_the_separate_call_trajectory_and_noise_moves_only_the_means(dev, deterministic):
    from brush_amd import TrainConfig

    quiet = dict(mcmc_noise_lr=0.0, mcmc_opacity_reg=0.0, mcmc_scale_reg=0.0, max_refine_step=0)
    base, _, _ = _run(dev, TrainConfig(warmup_steps=5, refine_every=10, max_refine_step=0, deferred_sh_adam=False), 6,
                      fused=False)
    off, _, tr = _run(dev, _mcmc_cfg(**quiet), 6)
    assert off == base and tr.last_refine is None
    # whatever fused_backward says
    off_fused, _, _ = _run(dev, _mcmc_cfg(**quiet), 2, fused=True)
    assert off_fused == base[:2]
    noisy, _, _ = _run(dev, _mcmc_cfg(**{**quiet, "mcmc_noise_lr": 5e5}), 1)
    assert noisy[0][0] != base[0][0]
    assert noisy[0][1:] == base[0][1:]
    # the regularisers reach Adam: its first moment (0.1 g after one step) changes, and with it, from the second step
    # on (the first moves every element by about its learning rate whatever |g| is), the scales and opacities
    reg, _, _ = _run(dev, _mcmc_cfg(**{**quiet, "mcmc_opacity_reg": 0.01, "mcmc_scale_reg": 0.01}), 2)
    assert reg[0][5] != base[0][5]
    assert reg[0][0] == base[0][0] and reg[0][2] == base[0][2] and reg[0][4] == base[0][4]
    assert reg[1][1] != base[1][1] and reg[1][3] != base[1][3]


def test_trainer_repeats_bitwise_refinements_included(dev, deterministic):
    a, sa, ta = _run(dev, _mcmc_cfg(), 32)
    b, sb, tb = _run(dev, _mcmc_cfg(), 32)
    assert sa.num_splats() == sb.num_splats() == 1100 and ta.opt_time == tb.opt_time == 32
    assert a == b


def test_steps_between_refinements_do_not_synchronise(dev):
    import torch

    from brush_amd import SplatTrainer

    cams, gts = _views(dev)
    splats = _splats(dev)
    tr = SplatTrainer(splats, _mcmc_cfg(warmup_steps=5, refine_every=50))
    tr.step(splats, cams[0], gts[0], 1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 21):  # iterations 1..20: past the warmup, before the first refinement (iteration 51)
            tr.step(splats, cams[i % 4], gts[i % 4], 1.0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert tr.last_refine is None and tr.iter == 21


def test_combinations(dev):
    import torch

    from brush_amd import SplatTrainer
    from brush_amd.pose import PoseTable

    cams, gts = _views(dev)
    splats = _splats(dev)
    tr = SplatTrainer(splats, _mcmc_cfg())
    with pytest.raises(ValueError, match="single-view"):
        tr.step(splats, cams[0], gts[0], 1.0, exchange=object())
    with pytest.raises(ValueError, match="single-view"):
        tr.step(splats, cams[0], gts[0], 1.0, grad_sync=lambda block, aux: None)
    assert tr.iter == 0
    for kw in (dict(antialiased=True), dict(pose=True)):
        splats = _splats(dev)
        poses = PoseTable(4, 1e-3, 5e-4, 1e-6) if kw.pop("pose", False) else None
        tr = SplatTrainer(splats, _mcmc_cfg(**kw))
        refines = 0
        for i in range(12):
            extra = {} if poses is None else dict(view_index=i % 4, poses=poses)
            loss, _, _ = tr.step(splats, cams[i % 4], gts[i % 4], 1.0, **extra)
            refines += tr.last_refine is not None
        assert refines == 1 and splats.num_splats() == 1050 and bool(torch.isfinite(loss).all())
        for k in PARAMS:
            assert bool(torch.isfinite(getattr(splats, k)).all()), k
        if poses is not None:
            poses.apply_all()
            assert bool(torch.isfinite(poses.delta).all()) and bool(poses.delta.abs().sum() > 0)


# ---------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    return TL._write_scene(str(tmp_path_factory.mktemp("mcmc_scene")), dev)


def test_train_scene_under_a_budget(dev, scene_dir):
    """The scene of test_gpu_train_loop.py under a budget of 3000 splats (the default strategy ends at ~25 800 and
    26.2-26.6 dB on it): growth of 5 % per refinement reaches the cap at the ninth.
    Measured on the MI355X at the defaults: 12.99 dB at step 0 -> 20.36 / 22.35 / 24.27 dB at steps 200 / 400 / 600 with
    2315 / 2811 / 3000 splats (+11.3 dB; the floor asks for +6, as the default strategy's test does).  The figures of
    each run go to profiles/mcmc_margins.json; the default strategy's on the same seed are in profiles/mcmc_e2e.json."""
    from brush_amd import TrainConfig
    from brush_amd.train_loop import load_dataset, train_scene

    data, _ = load_dataset(scene_dir)
    rows = []
    cfg = TrainConfig(strategy="mcmc", warmup_steps=50, refine_every=50, mcmc_cap_max=3000)
    splats, log = train_scene(data, cfg, steps=600, init_count=2000, sh_degree=3, seed=5, eval_every=200,
                              on_eval=lambda r, s: rows.append(r))
    print("mcmc e2e psnr by step:", [(r.step, round(r.psnr, 3), r.splats) for r in rows])
    MARGINS["e2e"] = {"psnr": [r.psnr for r in rows], "splats": [r.splats for r in rows],
                      "loss_first50_last50": [float(np.mean(log.losses[:50])), float(np.mean(log.losses[-50:]))]}
    assert [r.step for r in rows] == [0, 200, 400, 600]
    assert all(r.splats <= 3000 for r in rows) and rows[0].splats == 2000
    assert rows[-1].splats == 3000 and splats.num_splats() == 3000 and log.num_splats == 3000
    assert log.losses.shape == (600,) and np.isfinite(log.losses).all()
    assert float(np.mean(log.losses[-50:])) < float(np.mean(log.losses[:50]))
    assert rows[-1].psnr > rows[0].psnr + 6.0


def test_cli_strategy_and_cap(scene_dir, tmp_path):
    out_ply, out_json = str(tmp_path / "out.ply"), str(tmp_path / "log.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "60", "--init-count", "1000",
                        "--strategy", "mcmc", "--cap-max", "1500", "--export", out_ply, "--json", out_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_json) as f:
        log = json.load(f)
    assert log["strategy"] == "mcmc" and log["cap_max"] == 1500 and len(log["losses"]) == 60
    with open(out_ply, "rb") as f:
        head = f.read(2000)
    vertices = int(re.search(rb"element vertex (\d+)", head).group(1))
    assert 0 < vertices <= 1500 and vertices == log["num_splats"]
