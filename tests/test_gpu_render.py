"""GPU parity of the forward+backward rasterizer through the C ABI (pytest -m gpu).

Three anchors:
  1. the reference's golden vectors at its own tolerances (render.rs:815-830);
  2. the CPU oracle on seeded clouds: every integer output bit-exact, floats within 1e-4;
  3. size-independent properties at the headline size (1 M splats @1080p).
"""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import helpers as H
from tests import margins as M

pytestmark = pytest.mark.gpu

PIX_TOL = 1e-4  # north-star tolerance on pixels (L-inf)
EPS32 = 2.0 ** -24  # f32 unit round-off


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True  # counterpart of the reference's -12345 buffer poison
    return torch.device("cuda:0")


def _camera(w, h, position=None, rotation_xyzw=None, center_uv=None):
    import brush_amd

    c = H.reference_test_camera(w, h)
    return brush_amd.Camera(position or c["position"], rotation_xyzw or c["rotation_xyzw"], c["fov_x"], c["fov_y"],
                            center_uv or c["center_uv"])


def _t(a, dev, grad=False):
    import torch

    t = torch.as_tensor(np.ascontiguousarray(a), device=dev)
    if grad:
        t.requires_grad_(True)
    return t


def _np_u32(t):
    return t.detach().cpu().numpy().astype(np.int32).view(np.uint32)


@pytest.mark.parametrize("case", ["tiny_case", "basic_case"])
def test_reference_golden(dev, case):
    """test_reference of render.rs:695-833 through Splats.render + autograd."""
    import torch

    import brush_amd

    d = H.load_case(case)
    h, w, _ = d["out_img"].shape
    splats = brush_amd.Splats.from_safetensors(d, dev)
    out, aux = splats.render(_camera(w, h), (w, h), False)
    V = aux.read_num_visible()
    assert V == d["means"].shape[0]
    perm = aux.global_from_compact_gid[:V].long().cpu().numpy()
    proj = aux.projected_splats.detach().cpu().numpy()

    def chk(name, a, b, rtol, atol):
        ok, err, bad = H.all_close_report(a, b, rtol, atol)
        assert ok, f"{case}:{name} max_abs_err={err} bad={bad}"

    chk("xys", proj[:V, 0:2], d["xys"][perm], 1e-4, 1e-10)
    chk("conics", proj[:V, 2:5], d["conics"][perm], 1e-4, 5e-7)
    out_rgb = out[..., :3]
    chk("out_img", out_rgb.detach().cpu().numpy(), d["out_img"], 1e-4, 1e-9)
    crab = torch.as_tensor(H.crab_rgb(), device=dev)
    loss = ((out_rgb - crab) ** 2).mean()
    loss.backward()
    g = lambda p: p.grad.detach().cpu().numpy()
    chk("v_xy", g(splats.xys_dummy), d["v_xy"], 1e-4, 1e-9)
    chk("v_opacities", g(splats.raw_opacity), d["v_opacities"], 1e-4, 1e-10)
    chk("v_coeffs", g(splats.sh_coeffs), d["v_coeffs"], 1e-4, 1e-9)
    chk("v_scales", g(splats.log_scales), d["v_scales"], 1e-4, 1e-9)
    chk("v_means", g(splats.means), d["v_means"], 1e-4, 1e-9)
    chk("v_quats", g(splats.rotation), d["v_quats"], 1e-1, 1e-1)


def test_renders_at_all(dev):
    """render.rs:652-693"""
    import torch

    import brush_amd

    n = 8
    cam = brush_amd.Camera([0, 0, 0], [0, 0, 0, 1], 0.5, 0.5, (0.5, 0.5))
    means = torch.zeros((n, 3), device=dev, requires_grad=True)
    xy = torch.zeros((n, 2), device=dev, requires_grad=True)
    log_scales = (torch.ones((n, 3), device=dev) * 2.0).requires_grad_(True)
    quats = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev).repeat(n, 1).requires_grad_(True)
    sh = torch.ones((n, 1, 3), device=dev, requires_grad=True)
    raw = torch.zeros((n,), device=dev, requires_grad=True)
    out, aux = brush_amd.render_splats(cam, (32, 32), means, xy, log_scales, quats, sh, raw, False)
    assert abs(float(out[..., :3].mean())) < 1e-5
    assert float(out[..., 3].mean()) == 0.0
    assert aux.read_num_visible() == 0 and aux.read_num_intersections() == 0
    out.mean().backward()
    for p in (means, xy, log_scales, quats, sh, raw):
        assert not bool(p.grad.any())


_ORACLE_CACHE = {}


def _run_pair(dev, cloud, w, h, sh_degree, max_intersects=None, v_out=None, camera=None, deterministic=None):
    """Run the GPU op and the oracle on identical inputs (the oracle gets the uniform words the
    GPU op actually used).  Returns (gpu dict, oracle dict)."""
    import torch

    import brush_amd
    from brush_amd.render import uniforms_to_numpy

    import time as _time
    _t0 = [_time.perf_counter()]

    def _mark(what):  # wall-clock of the test's own phases (shown with -s): where a 20 M-splat case spends its minutes
        now = _time.perf_counter()
        print(f"[_run_pair n={cloud['means'].shape[0]}] {what}: {now - _t0[0]:.1f} s")
        _t0[0] = now

    params = {k: _t(cloud[k], dev, grad=True) for k in ("means", "log_scales", "quats", "sh", "raw_opac")}
    xy = torch.zeros((cloud["means"].shape[0], 2), device=dev, requires_grad=True)
    out, aux = brush_amd.render_splats(camera or _camera(w, h), (w, h), params["means"], xy, params["log_scales"],
                                       params["quats"], params["sh"], params["raw_opac"], False, max_intersects,
                                       deterministic=deterministic)
    u = uniforms_to_numpy(aux)
    default_v_out = v_out is None
    if default_v_out:
        rng = np.random.default_rng(7)
        v_out = (rng.standard_normal((h, w, 4)).astype(np.float32)) / np.float32(h * w)
    out.backward(_t(v_out, dev))
    # The oracle's own forward and end-to-end backward depend on the inputs only: the deterministic-mode module runs
    # every parity case a second time in the same process (and the c3 cloud at the reference cap twice), so they are
    # kept per (inputs fingerprint, uniforms, capacity) for the largest few cases instead of being recomputed.
    key = None
    if default_v_out:
        import hashlib
        hh = hashlib.sha1()
        for k in ("means", "log_scales", "quats", "sh", "raw_opac"):
            a = np.ascontiguousarray(cloud[k])
            hh.update(str(a.shape).encode()), hh.update(a[:4096].tobytes()), hh.update(a[-4096:].tobytes())
        hh.update(repr(sorted((k, np.asarray(v).tobytes()) for k, v in u.items())).encode())
        key = (hh.hexdigest(), int(aux.max_intersects), w, h)
    if key is not None and key in _ORACLE_CACHE:
        o_out, o_aux, o_g = _ORACLE_CACHE[key] = _ORACLE_CACHE.pop(key)  # (most recently used last)
    else:
        o_out, o_aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                        cloud["raw_opac"], max_intersects=aux.max_intersects)
        # End-to-end oracle gradients (oracle forward state) ...
        o_g = O.render_backward(u, o_aux, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["raw_opac"],
                                o_out, v_out)
        if key is not None and 200_000 <= cloud["means"].shape[0] <= 4_000_000:
            while len(_ORACLE_CACHE) >= 8:  # < 1 GB of host memory in all
                _ORACLE_CACHE.pop(next(iter(_ORACLE_CACHE)))
            _ORACLE_CACHE[key] = (o_out, o_aux, o_g)
    # ... and the backward in isolation: the oracle's backward fed with the forward state the GPU
    # backward consumed (the GPU's out_img and final_index).  The reference recovers
    # T_final = 1 - out.a (rasterize_backwards.wgsl:163), so on nearly opaque pixels a 1-ulp
    # difference in out.a (v_exp_f32 vs libm) is a ~1e-4 relative difference in T_final and in
    # every v_alpha term; sharing the forward state removes that amplification from the check.
    _mark("GPU fwd+bwd, oracle forward + end-to-end backward")
    g_out = out.detach().cpu().numpy()
    shared_aux = dict(o_aux)
    shared_aux["final_index"] = _np_u32(aux.final_index)
    # The same shared forward state through (a) the oracle with every sum in f32 as well (one admissible execution
    # of the reference's own arithmetic) and (b) the f64 arbiter: how far each f32 result is from the exact value.
    o_g_f32 = O.render_backward(u, shared_aux, cloud["means"], cloud["log_scales"], cloud["quats"],
                                cloud["raw_opac"], g_out, v_out, f32_sums=True)
    _mark("oracle backward on the shared forward state, f32 sums")
    o_g_f64 = O.render_backward_f64(u, shared_aux, cloud["means"], cloud["log_scales"], cloud["quats"],
                                    cloud["raw_opac"], g_out, v_out)
    _mark("f64 arbiter, shared forward state")
    # End to end through the arbiter as well: the f64 backward on the ORACLE's forward state, told per pixel how far the
    # GPU's forward state is from it.  Every term of a pixel is proportional to T_final = 1 - out.a
    # (rasterize_backwards.wgsl:163,173), so a relative difference dT / T of a pixel moves each of its terms by that
    # fraction: weight = 3 |T_gpu - T_oracle| / min(T) where both forwards stopped at the same entry.  Where they did not
    # (the saturation stop of rasterize.wgsl:88-91 sits within rounding of its threshold) T_final differs by the
    # skipped entries' (1 - alpha) factors, which cancel again in every T the backward recovers; what does differ is
    # the set of entries walked, so the arbiter is given both final_index maps and prices the entries in between.
    T_g = 1.0 - g_out[..., 3].astype(np.float64)
    T_o = 1.0 - o_out[..., 3].astype(np.float64)
    fin_g = _np_u32(aux.final_index)
    weight = np.where(fin_g == o_aux["final_index"], 3.0 * np.abs(T_g - T_o) / np.maximum(np.minimum(T_g, T_o), 1e-5), 0.0)
    o_g_f64_e2e = O.render_backward_f64(u, o_aux, cloud["means"], cloud["log_scales"], cloud["quats"],
                                        cloud["raw_opac"], o_out, v_out, pix_weight=weight, final_index_alt=fin_g,
                                        out_img_alt=g_out)
    _mark("f64 arbiter, end to end")
    gpu = dict(out=g_out, aux=aux, u=u,
               v_means=params["means"].grad, v_scales=params["log_scales"].grad, v_quats=params["quats"].grad,
               v_sh=params["sh"].grad, v_opac=params["raw_opac"].grad, v_xy=xy.grad)
    return gpu, dict(out=o_out, aux=o_aux, grads=o_g, grads_f32=o_g_f32, grads_f64=o_g_f64,
                     grads_f64_e2e=o_g_f64_e2e)


def _arbiter_report(gpu, orc, tag=""):
    """|gpu - f64| next to |oracle_f32 - f64| per gradient tensor (max and rms, in units of the tensor's scale)."""
    rep = {}
    for name in ("v_means", "v_scales", "v_quats", "v_sh", "v_opac", "v_xy"):
        t = orc["grads_f64"][name]
        a = gpu[name].detach().cpu().numpy().astype(np.float64).reshape(t.shape)
        r = orc["grads_f32"][name].astype(np.float64).reshape(t.shape)
        sc = np.abs(t).max() + 1e-300
        eg, er = np.abs(a - t), np.abs(r - t)
        rep[name] = dict(scale=sc, gpu_max=eg.max() / sc, gpu_rms=np.sqrt((eg ** 2).mean()) / sc,
                         ref_max=er.max() / sc, ref_rms=np.sqrt((er ** 2).mean()) / sc)
        mag = orc["grads_f64"]["mag_" + name[2:]]
        nz = mag > 0
        unit = EPS32 * mag[nz]
        rep[name].update(gpu_units=float((eg[nz] / unit).max()) if nz.any() else 0.0,
                         ref_units=float((er[nz] / unit).max()) if nz.any() else 0.0)
        print(f"[arbiter {tag}] {name}: scale {sc:.3e}  gpu max {rep[name]['gpu_max']:.2e} rms {rep[name]['gpu_rms']:.2e}"
              f"  | oracle-f32 max {rep[name]['ref_max']:.2e} rms {rep[name]['ref_rms']:.2e}"
              f"  | in eps*mag units: gpu {rep[name]['gpu_units']:.1f} oracle-f32 {rep[name]['ref_units']:.1f}")
    return rep


def _assert_forward_parity(gpu, orc, w, h, saturation_flip_frac=0.0, named=False, rounding_flips=False):
    """named: one of the scenes BASELINE.json names (S1, S4 / c1, c2, c3): on top of the conditioning-aware allowance
    the HARD ceilings hold there — max |gpu - f64| <= 1e-4 flat (the north-star's L-inf figure, no allowance), no
    pixel whose allowance exceeds 2e-4 and at most 1e-3 of the pixels above 1.2e-4 (so the allowance cannot quietly
    become the test), at most 2e-3 of the pixels inside a threshold guard band."""
    aux, oa = gpu["aux"], orc["aux"]
    # integer / index outputs: bit-exact (the checker tests/test_gpu_binning.py shares)
    V, I = BK.assert_integer_parity(BK.aux_arrays(aux, gpu["u"]["num_visible"]), oa)
    _assert_pixel_parity(gpu, orc, saturation_flip_frac, named, rounding_flips)
    return V, I


def _rounding_flip_explains(px_gpu, fin_gpu, x, y, oa, tol):
    """Is the GPU's pixel (rgba and final_index) the f64 composite of its tile's list under decisions that an f32
    evaluation may take?  The oracle's guard band (flip_risk) is 1e-5 relative around `alpha >= 1/255` and the stop test,
    the rounding of exp().  It does not know that sigma = 0.5 (a dx^2 + c dy^2) + b dx dy is itself only good to ~3 eps32
    of its CANCELLING terms (the figure of the pixel allowance above): on a thin tilted splat those terms are thousands
    of times sigma, alpha moves by 1e-4..1e-2 relative between two admissible f32 evaluations (with or without fused
    multiply-adds), and an entry at alpha ~ 1/255 is taken by one and dropped by the other.  Here every entry whose
    test sits inside ITS OWN band, 1e-5 + 3 eps32 (|t1| + |t2| + |t3|), may fall either way, the stop test may move by
    the band its transmittance has accumulated, and the pixel passes only if one of those executions reproduces the
    GPU's rgba within the unchanged pixel tolerance AND its final_index exactly."""
    tbx = oa["tile_bins"].shape[1]
    r0, r1 = (int(v) for v in oa["tile_bins"].reshape(-1, 2)[(y // 16) * tbx + x // 16])
    m = r1 - r0
    if m <= 0:
        return False
    p = oa["projected_splats"][oa["compact_gid_from_isect"][r0:r1]].astype(np.float64)
    dx, dy = p[:, 0] - (x + 0.5), p[:, 1] - (y + 0.5)
    t1, t2, t3 = 0.5 * p[:, 2] * dx * dx, 0.5 * p[:, 4] * dy * dy, p[:, 3] * dx * dy
    sg = t1 + t2 + t3
    band = 1e-5 + 3.0 * EPS32 * (np.abs(t1) + np.abs(t2) + np.abs(t3))  # of sigma (absolute) = of alpha (relative)
    with np.errstate(over="ignore"):
        a_u = p[:, 8] * np.exp(-sg)
    a = np.minimum(0.999, a_u)
    base = (sg >= 0.0) & (a_u >= 1.0 / 255.0)
    cand = ((np.abs(a_u * 255.0 - 1.0) <= band) & (sg >= -band)) | ((np.abs(sg) <= band) & (a_u * 255.0 >= 1.0 - band))
    # entries behind both walks' last entry decide nothing
    nxt = np.cumprod(np.where(base, 1.0 - a, 1.0))
    stops = np.flatnonzero(base & (nxt <= 1e-4 * (1.0 - 1e-3)))
    limit = max(int(stops[0]) if stops.size else m, int(fin_gpu) - r0 + 1)
    cand = np.flatnonzero(cand[:limit])
    k = cand.size
    if k > 4:  # 16 executions at most: far too few to come near an arbitrary colour (measured: k is 0 or 1)
        return False
    C = 1 << k
    passes = np.repeat(base[None, :], C, axis=0)
    passes[:, cand] ^= ((np.arange(C)[:, None] >> np.arange(k)[None, :]) & 1).astype(bool)
    fac = np.where(passes, 1.0 - a, 1.0)
    next_T = np.cumprod(fac, axis=1)
    T_acc = 1e-5 + np.cumsum(np.where(passes, a / (1.0 - a) * (band + 2.0 * EPS32), 0.0), axis=1)  # relative, of T
    rel = next_T / 1e-4 - 1.0
    for c in range(C):
        # the stop may fall on any passing entry from the first whose next_T can be <= 1e-4 to the first whose must be
        may = np.flatnonzero(passes[c] & (rel[c] <= T_acc[c]))
        must = np.flatnonzero(passes[c] & (rel[c] < -T_acc[c]))
        last = int(must[0]) if must.size else m
        for first in [int(v) for v in may[may <= last]] + ([m] if last == m else []):
            live = passes[c].copy()
            live[first:] = False
            wgt = np.where(live, a * (next_T[c] / fac[c]), 0.0)
            rgba = np.append(wgt @ p[:, 5:8], 1.0 - np.where(live, fac[c], 1.0).prod())
            on = np.flatnonzero(live)
            fin = r0 + int(on[-1]) if on.size else 0
            if fin == int(fin_gpu) and np.abs(rgba - px_gpu).max() <= tol:
                return True
    return False


def _assert_pixel_parity(gpu, orc, saturation_flip_frac=0.0, named=False, rounding_flips=False):
    """The float half of _assert_forward_parity: the composited image and final_index.
    rounding_flips (tests/test_gpu_binning.py: clouds with thin tilted splats at high opacity): a pixel that misses the
    tolerance or the oracle's final_index is first put to _rounding_flip_explains; one it explains joins the guard band,
    whose total is held to the bound the oracle's own band has.  Everything else is asserted as without it."""
    aux, oa = gpu["aux"], orc["aux"]
    # composite: 1e-4 L-inf away from pixels where a threshold test is within 1e-5 of flipping, measured against the
    # f64 evaluation of the same walk (same f32 records, same decisions).  Where the quadratic form cancels heavily (a
    # splat tens of thousands of pixels wide, far off-screen) any f32 evaluation of sigma is off by up to ~3 eps32 of
    # the CANCELLING terms — with or without the fused multiply-adds the reference leaves to its shader compiler — so
    # the allowance grows with the f64 pass's first-order sensitivity `cond` to exactly that (found by
    # tests/fuzz_parity.py with the camera inside a dense cloud: the GPU and the f32 restatement are equally far from
    # f64 there, 1.2e-4 / 1.5e-4 at the 99th percentile, and 6e-4 from each other; on the bench scenes cond is small
    # and this is the plain 1e-4 test).
    risk = oa["flip_risk"].astype(bool)
    # how many pixels may sit inside a guard band: each of a pixel's entries lands within 1e-5 relative of a threshold
    # with probability ~2e-5, so the bound grows with the depth of the lists (it means little on a thumbnail either)
    lens = (oa["tile_bins"][..., 1].astype(np.int64) - oa["tile_bins"][..., 0].astype(np.int64)).reshape(-1)
    depth = float(lens[lens > 0].mean()) if (lens > 0).any() else 0.0
    assert risk.mean() < 2e-3 + 2e-5 * depth or risk.sum() <= 16, (float(risk.mean()), depth)
    if named:
        assert risk.mean() < 2e-3, float(risk.mean())
    diff = np.abs(gpu["out"] - orc["out"]).max(axis=2)
    exact, cond = O.rasterize_forward_f64(gpu["u"], oa)
    gpu_err = np.abs(gpu["out"].astype(np.float64) - exact).max(axis=2)
    tol = PIX_TOL + 3.0 * EPS32 * cond
    if rounding_flips:
        fin_gpu = _np_u32(aux.final_index)
        suspects = ((gpu_err > tol) | (fin_gpu != oa["final_index"])) & ~risk
        explained = np.zeros_like(risk)
        if suspects.mean() < 2e-3 + 2e-5 * depth or suspects.sum() <= 16:  # more than a guard band may hold: no excuse
            for y, x in zip(*np.nonzero(suspects)):
                explained[y, x] = _rounding_flip_explains(gpu["out"][y, x].astype(np.float64), fin_gpu[y, x], int(x),
                                                          int(y), oa, float(tol[y, x]))
        print(f"pixels off the tolerance or the oracle's final_index outside its guard band: {int(suspects.sum())}, "
              f"of which an f32 rounding of sigma at a threshold explains {int(explained.sum())}")
        risk = risk | explained
        assert risk.mean() < 2e-3 + 2e-5 * depth or risk.sum() <= 16, (float(risk.mean()), depth)
    over = (gpu_err > tol) & ~risk
    assert not over.any(), (f"{int(over.sum())} pixels: max |gpu - f64| {gpu_err[over].max()} (allowance {tol[over].min()}); "
                            f"max |gpu - f32 restatement| {diff[~risk].max()}")
    print(f"pixels: max |gpu - f64| {gpu_err[~risk].max():.2e}, median allowance {np.median(tol):.2e}, max {tol.max():.2e}, "
          f"pixels whose allowance exceeds 2e-4: {int((tol > 2e-4).sum())} of {tol.size}")
    pix_ratio = float((gpu_err / tol)[~risk].max()) if (~risk).any() else 0.0
    M.record("pixels", "summary", dict(worst=pix_ratio, max_gpu_minus_f64=float(gpu_err[~risk].max()), allowance_max=float(tol.max()),
                                       allowance_median=float(np.median(tol)), over_2e_4=int((tol > 2e-4).sum()),
                                       flip_risk_frac=float(risk.mean()), max_gpu_minus_f32_restatement=float(diff[~risk].max()),
                                       named=bool(named)))
    M.check_growth("pixels", "summary", pix_ratio)
    if named:
        assert gpu_err[~risk].max() <= PIX_TOL, gpu_err[~risk].max()
        assert not (tol > 2e-4).any(), f"named scene: pixel allowance reaches {tol.max():.3e}"
        assert (tol > 1.2e-4).mean() <= 1e-3, float((tol > 1.2e-4).mean())
    assert diff.max() <= 2.0 / 255.0 + 2.0 * tol.max()
    fi = _np_u32(aux.final_index)
    differ = (fi != oa["final_index"]) & ~risk
    if saturation_flip_frac == 0.0:
        assert not differ.any()
    else:
        # Deep lists (hundreds of entries per pixel): the transmittance is a product of hundreds of (1 - alpha)
        # factors, so its relative rounding error outgrows the oracle's 1e-5 guard band around the
        # `T(1-alpha) <= 1e-4` stop test (rasterize.wgsl:88-91).  A flipped stop moves final_index by a few
        # entries on a pixel that is saturated either way: bound how many there are and check that they are
        # exactly that case (both alphas at the saturation level, colours within the pixel tolerance already
        # asserted above).
        print(f"final_index differs off the guard band on {int(differ.sum())} of {differ.size} pixels")
        assert differ.mean() <= saturation_flip_frac
        if differ.any():
            assert gpu["out"][..., 3][differ].min() >= 0.9998 and orc["out"][..., 3][differ].min() >= 0.9998


# Gradient tolerance, element by element, every term tied to a mechanism (no "fraction of the tensor's maximum"):
#   |gpu - f64| <= RTOL |f64|                      the reference's own rtol (render.rs:815-830)
#                + C_TERM eps32 mag               mag = sum of the MAGNITUDES of the per-pixel terms the element is
#                                                 made of (f64 arbiter, carried through |gather / projection VJP|):
#                                                 a per-term relative accuracy of C_TERM eps32, whatever the
#                                                 summation order (v_exp_f32 + f32 exponent argument: ~5 eps per
#                                                 alpha)
#                + C_DEPTH eps32 dep              dep = the same terms, each weighted by the roundings (in eps) its
#                                                 recovered T has gone through: T is T_final divided by the f32
#                                                 (1 - alpha) of every entry walked so far
#                                                 (rasterize_backwards.wgsl:244-246), one rounding per division plus
#                                                 alpha / (1 - alpha) <= 99 for the cancellation in 1 - alpha: on a
#                                                 list hundreds of entries deep the rounding of T, not of the term,
#                                                 is what limits an f32 evaluation
#                + C_FLIP flip                    what the threshold decisions that sit within f32 rounding of
#                                                 flipping (alpha ~ 1/255, sigma ~ 0) can move (arbiter)
#                + C_VJP eps32 vjp                the rounding noise of the per-splat VJP itself (v_sh: the terms of the
#                                                 SH basis polynomial, which passes through zero; v_opac: the (1 - s)
#                                                 of a saturating sigmoid); v_means / v_scales / v_quats: the
#                                                 projection VJP; vjp = the sum of the magnitudes of the terms
#                                                 it adds up (terms of size scale^2 cancel in v_V = T^t v_cov T and in
#                                                 the column dot products of v_scale), evaluated by the arbiter.  The
#                                                 GPU runs the same expression trees (-ffp-contract=off) on inputs that
#                                                 differ in the last bits, so its noise is a different sample of it.
#                + C_REF rowmax|oracle_f32 - f64| the error the f32 restatement of the reference makes on this row
# The constants are CALIBRATED, not guessed: every run evaluates the candidate sets below and records each one's worst
# err/tol per test and tensor (profiles/parity_margins.json).  Measured over the whole suite in both modes: with
# (C_TERM, C_DEPTH, C_VJP, C_REF) = (8, 1, 8, 1) the worst ratio over the elements WITHOUT a flip allowance is 0.24 on
# every test whose scene the reference itself can run (each constant at most 4x what was ever observed; round 2 used
# (64, -, 16, 4)); the 20 M-splat 4K frame (c5: lists 556 entries deep, beyond the reference's limits) needs C_DEPTH = 2
# (1.06 with 1), so 2 it is: no-flip worst 0.69 there.  On top of the allowance, no test's worst ratio may grow past 2x
# its tracked value
# (tests/margins.py): a kernel change that makes the gradients several times less accurate turns the suite red even
# though it still fits the mechanism-based bound (BRUSH_INJECT_VVA_ULPS build, tests/test_gpu_gate.py).
# C_FLIP: `flip` is what the decisions at risk CAN move (an upper bound by construction, priced entry by entry by the
# arbiter: the entry's own terms, alpha / (1 - alpha) of the later terms of its pixel and, since round 4, for a stop
# that fell on different entries in the two forward states, the skipped entries' actual colour in the accumulator and
# their factors in T_final).  Round 3 needed 1.5 x that bound on the 20 M-splat frame (err = 1.53 x flip on five
# tensors): the stop mismatch was priced in units of the later entry's own colour.  The candidates below carry C_FLIP
# as their fifth constant so that every run records what each value would have given.
RTOL = 1e-4
CANDIDATES = {                      # (C_TERM, C_DEPTH, C_VJP, C_REF, C_FLIP)
    "r2": (64.0, 0.0, 16.0, 4.0, 1.5),   # round 2's set (no depth term, the f32 restatement's own error x 4)
    "a": (8.0, 1.0, 8.0, 1.0, 1.5),
    "b": (8.0, 0.5, 8.0, 1.0, 1.5),
    "c": (4.0, 1.0, 4.0, 1.0, 1.5),
    "d": (4.0, 0.5, 4.0, 0.0, 1.5),
    "e": (8.0, 1.0, 8.0, 0.0, 1.5),
    "f": (4.0, 0.25, 4.0, 1.0, 1.5),
    "g": (8.0, 0.25, 8.0, 1.0, 1.5),
    "h": (8.0, 2.0, 8.0, 1.0, 1.5),      # round 3's set
    "i": (4.0, 2.0, 4.0, 1.0, 1.5),
    "h1": (8.0, 2.0, 8.0, 1.0, 1.0),
    "h075": (8.0, 2.0, 8.0, 1.0, 0.75),
    "h05": (8.0, 2.0, 8.0, 1.0, 0.5),
    "h025": (8.0, 2.0, 8.0, 1.0, 0.25),
}
ACTIVE = "h1"
C_TERM, C_DEPTH, C_VJP, C_REF, C_FLIP = CANDIDATES[ACTIVE]
GRAD_NAMES = ("v_means", "v_scales", "v_quats", "v_sh", "v_opac", "v_xy")


def _grad_ratio(a, f64, f32_err_rowmax, name, consts):
    """err / tol per element of one tensor for one constant set; returns (ratio, err, parts)."""
    c_term, c_dep, c_vjp, c_ref, c_flip = consts
    t = f64[name]
    mag, flip, dep = f64["mag_" + name[2:]], f64["flip_" + name[2:]], f64["dep_" + name[2:]]
    vjp = f64.get("vjp_" + name[2:], 0.0)
    parts = (RTOL * np.abs(t), EPS32 * (c_term * mag + c_dep * dep), c_flip * flip, c_vjp * EPS32 * vjp + 0.0 * mag,
             c_ref * f32_err_rowmax)
    tol = parts[0] + parts[1] + parts[2] + parts[3] + parts[4] + 1e-300
    err = np.abs(a - t)
    return err / tol, err, parts


def _rowmax(x, shape):
    n = shape[0]
    return x.reshape(n, -1).max(axis=1).reshape((n,) + (1,) * (len(shape) - 1)) if n else x


def _assert_grad_parity(gpu, orc, tag=""):
    """GPU gradients against the f64 arbiter, element by element, twice: fed with the forward state the GPU backward
    consumed (`shared`), and end to end against the arbiter on the oracle's own forward state with the measured
    per-pixel difference of the two forward states folded into the flip allowance (`e2e`, see _run_pair; T_final =
    1 - out.a turns a 1-ulp difference of out.a into 1e-4 of T on nearly opaque pixels — inherent to the reference's
    formulation, and now priced per element instead of by a fraction of the tensor's maximum).  Plus exact zeros off
    the visible set.  Records every margin (tests/margins.py) and asserts none has grown past 2x its tracked value."""
    import torch

    V = int(orc["aux"]["num_visible"][0])
    worst = {}
    # Everything below runs on the rows of the VISIBLE splats only (~10 % of a cloud): off the visible set the GPU's
    # gradients and both references must be exact zeros, which is asserted on the whole arrays first (one cheap pass
    # each); the per-element gate then sees the same worst ratios as on the full arrays (a zero row has err 0) at a tenth
    # of the float64 temporaries — the 20 M-splat case spent 220 of its 245 s here.
    n_all = gpu["v_means"].shape[0]
    vis_rows = np.sort(orc["aux"]["global_from_compact_gid"][:V].astype(np.int64))
    vis_mask = np.zeros(n_all, bool)
    vis_mask[vis_rows] = True
    vis_mask_t = torch.as_tensor(vis_mask, device=gpu["v_means"].device)
    vis_rows_t = torch.as_tensor(vis_rows, device=gpu["v_means"].device)

    def rows_of(x):
        return x[vis_rows] if isinstance(x, np.ndarray) and x.ndim >= 1 and x.shape[0] == n_all else x

    def zero_off_visible(x):
        flat = x.reshape(n_all, -1)
        return not np.count_nonzero(flat[~vis_mask]) if flat.shape[0] else True

    for leg, f64_all, f32_ref in (("shared", orc["grads_f64"], orc["grads_f32"]), ("e2e", orc["grads_f64_e2e"], orc["grads"])):
        for name in GRAD_NAMES:
            if leg == "shared":  # dense and exactly zero for non-visible splats
                assert not bool(gpu[name].detach().reshape(n_all, -1)[~vis_mask_t].any()), name
            assert zero_off_visible(f64_all[name]) and zero_off_visible(f32_ref[name]), (leg, name)
            f64 = {k: rows_of(v) for k, v in f64_all.items() if k == name or k.endswith("_" + name[2:])}
            t = f64[name]
            a = gpu[name].detach().reshape(n_all, -1)[vis_rows_t].cpu().numpy().astype(np.float64).reshape(t.shape)
            ref_err = np.abs(rows_of(f32_ref[name].reshape((n_all,) + t.shape[1:])).astype(np.float64) - t)
            row_ref = _rowmax(ref_err, t.shape)
            flip = f64["flip_" + name[2:]]
            rec = {}
            for key, consts in CANDIDATES.items():
                ratio, err, parts = _grad_ratio(a, f64, row_ref, name, consts)
                noflip = ratio[flip == 0] if ratio.size else ratio
                rec[key] = dict(worst=float(ratio.max()) if ratio.size else 0.0,
                                worst_noflip=float(noflip.max()) if noflip.size else 0.0)
                if key == ACTIVE:
                    active = (ratio, err, parts)
            ratio, err, parts = active
            i = int(np.argmax(ratio)) if ratio.size else 0
            w = float(ratio.reshape(-1)[i]) if ratio.size else 0.0
            worst[(leg, name)] = w
            mag = f64["mag_" + name[2:]]
            nz = (mag > 0) & (flip == 0)
            units = float((err[nz] / (EPS32 * mag[nz])).max()) if nz.any() else 0.0
            entry = dict(worst=w, units_eps_mag_noflip=units, candidates=rec, elements_with_flip=int((flip > 0).sum()))
            if ratio.size:
                pv = [float(np.broadcast_to(x, t.shape).reshape(-1)[i]) for x in parts]
                entry.update(err=float(err.reshape(-1)[i]), parts=dict(rtol=pv[0], term=pv[1], flip=pv[2], vjp=pv[3], ref=pv[4]))
                print(f"[grad {leg} {tag}] {name}: worst err/tol {w:.3f} (err {entry['err']:.3e}; tol parts rtol {pv[0]:.2e} "
                      f"term {pv[1]:.2e} flip {pv[2]:.2e} vjp {pv[3]:.2e} ref {pv[4]:.2e}); max err/(eps mag) off the flip "
                      f"elements {units:.1f}; " + " ".join(f"{k}:{v['worst']:.2f}/{v['worst_noflip']:.2f}" for k, v in rec.items()))
            M.record("grad_" + leg, name, entry)
            assert (ratio <= 1.0).all(), f"{leg} {name}: worst err/tol {w:.3f}, {(ratio > 1.0).sum()} elements over"
            M.check_growth("grad_" + leg, name, w)
    return worst


@pytest.mark.parametrize("n,w,h,deg,mult", [
    (2000, 123, 82, 3, 0.002),       # ragged image (not a tile multiple), every SH band
    (20000, 256, 192, 0, 0.01),
    (20000, 200, 120, 1, 0.01),
    (20000, 200, 120, 2, 0.01),
    (20000, 200, 120, 4, 0.01),
    (150000, 640, 480, 3, 0.05),     # long tile lists (multiple LDS batches)
    (300000, 800, 800, 0, 1.0),      # c2-sized, bench distribution
])
def test_matches_oracle(dev, n, w, h, deg, mult):
    cloud = H.synthetic_cloud(n, deg, seed=4, mean_mult=mult)
    gpu, orc = _run_pair(dev, cloud, w, h, deg, max_intersects=4_000_000)
    V, I = _assert_forward_parity(gpu, orc, w, h)
    assert V > 0 and I > 0
    _arbiter_report(gpu, orc, f"{n}@{w}x{h}")
    _assert_grad_parity(gpu, orc, f"{n}@{w}x{h}")


def test_rotated_off_centre_camera(dev):
    """Non-identity world->camera rotation, translated eye, principal point off centre: exercises every
    element of the 28-word uniforms (viewmat columns, pixel_center) against the oracle."""
    q = np.array([0.12, -0.31, 0.07, 0.0])
    q[3] = np.sqrt(1.0 - (q[:3] ** 2).sum())
    cam = _camera(200, 120, position=[1.5, -0.7, -6.0], rotation_xyzw=q.tolist(), center_uv=(0.43, 0.58))
    cloud = H.synthetic_cloud(20000, 2, seed=11, mean_mult=0.01)
    gpu, orc = _run_pair(dev, cloud, 200, 120, 2, camera=cam)
    V, I = _assert_forward_parity(gpu, orc, 200, 120)
    assert V > 1000 and I > V
    _assert_grad_parity(gpu, orc)


def test_alpha_clamp_quirk(dev):
    """Opacities ~1: alpha reaches the 0.999 forward clamp but the backward clamps at 0.99
    (rasterize.wgsl:83 vs rasterize_backwards.wgsl:239).  The GPU must reproduce that mismatch: the
    oracle follows the WGSL text, and a backward using 0.999 would be off by far more than the
    tolerance on the saturated pixels."""
    cloud = H.synthetic_cloud(3000, 0, seed=21, mean_mult=0.002)
    cloud["raw_opac"][:] = 12.0  # sigmoid -> 0.999994
    gpu, orc = _run_pair(dev, cloud, 160, 96, 0)
    _assert_forward_parity(gpu, orc, 160, 96)
    proj = orc["aux"]["projected_splats"][: int(orc["aux"]["num_visible"][0])]
    assert (proj[:, 8] > 0.9999).all()
    _assert_grad_parity(gpu, orc)
    # sanity: the quirk is active (a 0.999-clamped backward differs visibly from the 0.99 one)
    assert np.abs(orc["grads"]["v_opac"]).max() > 0


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_tiny_and_empty_inputs(dev, n):
    """Empty and ragged splat counts (the reference allocates [0,..] tensors without complaint)."""
    import torch

    import brush_amd

    cloud = H.synthetic_cloud(max(n, 1), 1, seed=5, mean_mult=0.0005)
    cloud = {k: v[:n] for k, v in cloud.items()}
    if n == 0:
        p = {k: _t(v, dev, grad=True) for k, v in cloud.items()}
        out, aux = brush_amd.render_splats(_camera(64, 48), (64, 48), p["means"], None, p["log_scales"], p["quats"],
                                           p["sh"], p["raw_opac"])
        assert aux.read_num_visible() == 0 and aux.read_num_intersections() == 0
        assert not bool(out.any())
        out.sum().backward()
        assert all(v.grad is not None and v.grad.numel() == 0 for v in p.values())
        assert not bool(aux.tile_bins.any())
        return
    gpu, orc = _run_pair(dev, cloud, 64, 48, 1)
    _assert_forward_parity(gpu, orc, 64, 48)
    _assert_grad_parity(gpu, orc)


@pytest.mark.parametrize("n,deg,w,h", [(1003, 3, 200, 120), (1001, 2, 64, 48), (70001, 0, 640, 480), (5, 4, 32, 32),
                                       (200003, 3, 32, 32)])  # last: > 1 MiB of zeros per tile, the VJP kernel keeps them
def test_dense_gradients_zeroed_in_passing(dev, n, deg, w, h):
    """The compositing backward zero-fills the dense gradient arrays beside its arithmetic (ZeroFill) and the VJP kernel
    writes the visible rows only: NaN-poisoned outputs must come back dense — exact zeros off the visible set, the same
    bits as the all-in-one VJP kernel on it — for splat counts that leave partial KiB blocks and 1-3 trailing floats in
    every array, in both accumulation modes; arrays that are not 16-byte aligned, and a cloud far too large for the
    frame's few waves, take the old path (zeros written by the VJP kernel) and must give the same bits."""
    import torch

    import brush_amd
    from brush_amd import render as R

    cloud = H.synthetic_cloud(n, deg, seed=11, mean_mult=0.002)
    p = {k: _t(v, dev) for k, v in cloud.items()}
    C = (deg + 1) ** 2
    cam = _camera(w, h)
    rng = np.random.default_rng(3)
    v_out = _t(rng.standard_normal((h, w, 4)).astype(np.float32) / np.float32(h * w), dev)
    layout, total = R.grad_block_layout(n, C)
    for det in (False, True):
        out, aux, u = R._forward_impl(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], False,
                                      None, deterministic=det)
        V = aux.read_num_visible()
        vis = torch.zeros(n, dtype=torch.bool, device=dev)
        vis[aux.global_from_compact_gid[:V].long()] = True
        runs = {}
        for name, shift in (("aligned", 0), ("unaligned", 1)):
            # guard floats of NaN around the block: the fill must not write outside the arrays either
            buf = torch.full((total + 16,), float("nan"), device=dev)
            block = buf[4 + shift:4 + shift + total]
            assert (block.data_ptr() % 16 == 0) == (shift == 0)
            g, _ = R._backward_impl(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], C, out, v_out, block)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:4 + shift]).all()) and bool(torch.isnan(buf[4 + shift + total:]).all())
            for off, sz in layout.values():  # the padding between the arrays of the block stays untouched as well
                assert bool(torch.isnan(block[off + sz:(off + sz + 3) // 4 * 4]).all())
            for k, t in g.items():
                assert not bool(torch.isnan(t).any()), (det, name, k)
                assert not bool(t[~vis].any()), (det, name, k)
            runs[name] = {k: t.clone() for k, t in g.items()}
        if det:  # bitwise reproducible mode: the two paths must agree to the bit
            for k in runs["aligned"]:
                assert torch.equal(runs["aligned"][k], runs["unaligned"][k]), k
        else:    # float atomics: the compositing sums differ in arrival order only
            for k in runs["aligned"]:
                a, b = runs["aligned"][k], runs["unaligned"][k]
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-6 * float(b.abs().max()) + 1e-30), k



@pytest.mark.parametrize("seed", range(10))
def test_dense_gradients_zeroed_in_passing_random_shapes(dev, seed):
    """Random splat counts / SH degrees / frame sizes through test_dense_gradients_zeroed_in_passing: every combination
    of partial last blocks, trailing floats, waves without a tile and tiles without records must leave dense arrays with
    exact zeros off the visible set and untouched guard words."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 40000))
    deg = int(rng.integers(0, 5))
    w, h = int(rng.integers(8, 500)), int(rng.integers(8, 300))
    test_dense_gradients_zeroed_in_passing(dev, n, deg, w, h)


def test_walk_queue_overflow_falls_back_inline(dev):
    """A handful of whole-screen splats need far more (splat, chunk) work items than the queue
    holds (capacity = N): the overflowing splats are walked inline and the result is unchanged."""
    n, w, h = 100, 1920, 1080  # 32 chunks per splat: only the first 3 reservations fit in 100 slots
    cloud = H.synthetic_cloud(n, 0, seed=2, mean_mult=0.0001)
    cloud["means"][:, 2] = np.linspace(-7.5, -6.5, n).astype(np.float32)  # 0.5..1.5 in front of the eye
    cloud["log_scales"][:] = np.log(4.0)
    gpu, orc = _run_pair(dev, cloud, w, h, 0, max_intersects=1_000_000)
    V, I = _assert_forward_parity(gpu, orc, w, h)
    assert V == n and I > 8160 * 8  # most splats cover the whole 120x68 tile grid
    _assert_grad_parity(gpu, orc)


def test_cloud_above_self_scan_limit(dev):
    """2.4 M splats: more than 2048 cull workgroups, i.e. the separate block-count scan launch instead
    of the in-compaction scan used for smaller clouds; forward state bit-exact against the oracle."""
    cloud = H.synthetic_cloud(2_400_000, 0, seed=7, mean_mult=1.0)
    gpu, orc = _run_pair(dev, cloud, 640, 360, 0, max_intersects=4_000_000)
    V, I = _assert_forward_parity(gpu, orc, 640, 360)
    assert V > 50000 and I > V
    _assert_grad_parity(gpu, orc)


def test_4k_frame(dev):
    """3840x2160 (240x135 tiles, 15-bit tile ids -> 16 sorted bits, SURVEY §8 c5 resolution)."""
    cloud = H.synthetic_cloud(120000, 0, seed=4, mean_mult=1.0)
    gpu, orc = _run_pair(dev, cloud, 3840, 2160, 0, max_intersects=3_000_000)
    V, I = _assert_forward_parity(gpu, orc, 3840, 2160)
    assert V > 5000 and I > V
    _assert_grad_parity(gpu, orc)


def test_depth_ties_are_deterministic(dev):
    """Equal depths: compaction keeps global order, so ties break by global id."""
    cloud = H.synthetic_cloud(4000, 0, seed=9, mean_mult=0.002)
    cloud["means"][:, 2] = np.round(cloud["means"][:, 2])  # many exact depth ties
    gpu, orc = _run_pair(dev, cloud, 160, 96, 0)
    _assert_forward_parity(gpu, orc, 160, 96)
    V = gpu["aux"].read_num_visible()
    gids = _np_u32(gpu["aux"].global_from_compact_gid)[:V]
    depth = (cloud["means"][gids, 2] + 8.0)
    same = depth[1:] == depth[:-1]
    assert same.sum() > 100 and (gids[1:][same] > gids[:-1][same]).all()


def test_intersection_overflow_is_flagged(dev):
    """The reference truncates silently (map_gaussian_to_intersects.wgsl:40); the build clamps
    num_intersections to the capacity and raises aux.overflow."""
    cloud = H.synthetic_cloud(5000, 0, seed=3, mean_mult=0.002)
    gpu, orc = _run_pair(dev, cloud, 160, 96, 0, max_intersects=1000)
    assert int(gpu["aux"].overflow.item()) == 1 and orc["aux"]["overflow"]
    assert gpu["aux"].read_num_intersections() == 1000
    _assert_forward_parity(gpu, orc, 160, 96)


def test_raster_u32(dev):
    """Packed RGBA8 path (rasterize.wgsl:106-109) vs the oracle, allowing 1 LSB where the
    float image differs by an exp() ulp."""
    import brush_amd

    cloud = H.synthetic_cloud(20000, 0, seed=4, mean_mult=0.01)
    w, h = 256, 192
    p = {k: _t(cloud[k], dev) for k in cloud}
    out, aux = brush_amd.render_splats(_camera(w, h), (w, h), p["means"], None, p["log_scales"], p["quats"], p["sh"],
                                       p["raw_opac"], True)
    assert tuple(out.shape) == (h, w, 1)
    from brush_amd.render import uniforms_to_numpy

    o_out, _ = O.render_forward(uniforms_to_numpy(aux), cloud["means"], cloud["log_scales"], cloud["quats"],
                                cloud["sh"], cloud["raw_opac"], raster_u32=True)
    a = _np_u32(out[..., 0])
    ch = lambda x, k: ((x >> (8 * k)) & 0xFF).astype(np.int32)
    for k in range(4):
        assert np.abs(ch(a, k) - ch(o_out, k)).max() <= 1
    assert (a == o_out).mean() > 0.99


def test_headline_size_matches_oracle(dev):
    """The headline configuration itself (1 048 576 splats @1920x1080, SH degree 3, the bench's seed):
    integer state bit-exact, pixels and gradients within the stated tolerances, against the oracle."""
    cloud = H.synthetic_cloud(1 << 20, 3, seed=4, mean_mult=1.0)
    gpu, orc = _run_pair(dev, cloud, 1920, 1080, 3)
    V, I = _assert_forward_parity(gpu, orc, 1920, 1080, named=True)
    _risk_report(orc, "S1")
    assert V > 100000 and I > 400000
    # per-element gate against the f64 arbiter (_assert_grad_parity: mechanism-based allowance, tracked margins); no
    # fraction of a tensor's scale enters it
    _assert_grad_parity(gpu, orc)


def test_dense_scene_matches_oracle(dev):
    """The bench's dense scene (1 048 576 splats @1920x1080, mean_mult 0.25, SH degree 3: 2.6 M intersections, tile lists
    of ~320 entries = five LDS batches per tile at one wave per tile) against the oracle and the f64 arbiter."""
    cloud = H.synthetic_cloud(1 << 20, 3, seed=4, mean_mult=0.25)
    gpu, orc = _run_pair(dev, cloud, 1920, 1080, 3)
    V, I = _assert_forward_parity(gpu, orc, 1920, 1080, named=True)
    _risk_report(orc, "dense")
    assert V > 100000 and I > 2_000_000
    _assert_grad_parity(gpu, orc)


def _risk_report(orc, tag):
    risk = orc["aux"]["flip_risk"].astype(bool)
    print(f"[{tag}] flip-risk pixels excluded from the 1e-4 / final_index checks: {int(risk.sum())} of {risk.size} "
          f"({100.0 * risk.mean():.4f} %)")


@pytest.mark.parametrize("n,w,h,deg", [
    (104_858, 400, 400, 3),    # S4 / config c1: lego.ply-sized cloud @400x400
    (314_573, 800, 800, 3),    # S4 / config c2: lego train @800x800, every SH band
])
def test_s4_sizes_match_oracle(dev, n, w, h, deg):
    """SURVEY §8(d) S4, the c1- and c2-sized synthetic stand-ins (no .ply / NeRF-synthetic data exists here)."""
    cloud = H.synthetic_cloud(n, deg, seed=4, mean_mult=1.0)
    gpu, orc = _run_pair(dev, cloud, w, h, deg)
    V, I = _assert_forward_parity(gpu, orc, w, h, named=True)
    _risk_report(orc, f"S4 {n}@{w}x{h}")
    assert V > 5000 and I > V
    _assert_grad_parity(gpu, orc)


@pytest.fixture(scope="module")
def c3_cloud():
    # config c3 (garden-scale): 3 M splats @1080p, SH degree 3.  mean_mult 0.12 packs the bench
    # distribution until the frame is saturated: V = 376 754, 27.0 M intersections (3.2x the reference's
    # 8 388 480 cap, render.rs:204-206), tile lists of 3300-4000 entries.
    return H.synthetic_cloud(3_000_000, 3, seed=4, mean_mult=0.12)


def test_c3_scale_raised_cap(dev, c3_cloud):
    """c3 with room for every intersection (max_intersects 40 M): integer state bit-exact, pixels and all six
    gradients against the oracle."""
    gpu, orc = _run_pair(dev, c3_cloud, 1920, 1080, 3, max_intersects=40_000_000)
    V, I = _assert_forward_parity(gpu, orc, 1920, 1080, named=True)
    _risk_report(orc, "c3 raised cap")
    assert V > 300_000 and I >= 20_000_000 and int(gpu["aux"].overflow.item()) == 0
    _assert_grad_parity(gpu, orc)


def test_c3_scale_reference_cap_overflows(dev, c3_cloud):
    """The same cloud at the reference's default capacity min(N*T, 128*65535): the reference truncates
    silently (map_gaussian_to_intersects.wgsl:40); the build truncates at the same place, raises
    aux.overflow and stays bit-exact with the oracle run at that capacity."""
    gpu, orc = _run_pair(dev, c3_cloud, 1920, 1080, 3)
    assert gpu["aux"].max_intersects == 128 * 65535
    V, I = _assert_forward_parity(gpu, orc, 1920, 1080, named=True)
    assert I == 8_388_480 and int(gpu["aux"].overflow.item()) == 1 and orc["aux"]["overflow"]
    _assert_grad_parity(gpu, orc)


@pytest.fixture(scope="module")
def c5_cloud():
    return H.synthetic_cloud(20_971_520, 1, seed=4, mean_mult=1.0)


C5_STATE = {}  # the SH-1 run of test_c5_scale_20m_splats_4k, kept for test_c5_sh_degree_3_equals_the_sh1_run


def test_c5_scale_20m_splats_4k(dev, c5_cloud):
    """config c5 / S3: 20 971 520 splats @3840x2160 (beyond the reference's 65 535-workgroup and
    8.39 M-intersection limits, so parity is against the oracle only): V = 2.04 M, I = 18.0 M, 32 400
    tiles (15-bit ids).  Integer state bit-exact, pixels within 1e-4, gradients against the oracle.  Run in
    deterministic mode: the worst ratios of this frame's 556-entry lists sit closest to their bounds, and with float
    atomics they move from run to run."""
    gpu, orc = _run_pair(dev, c5_cloud, 3840, 2160, 1, max_intersects=24_000_000, deterministic=True)
    V, I = _assert_forward_parity(gpu, orc, 3840, 2160, saturation_flip_frac=1e-4)
    _risk_report(orc, "c5")
    assert V > 2_000_000 and I > 17_000_000 and int(gpu["aux"].overflow.item()) == 0
    C5_STATE.update(out=gpu["out"], aux=gpu["aux"], u=gpu["u"],
                    grads={k: gpu[k].detach().clone() for k in GRAD_NAMES})
    _assert_grad_parity(gpu, orc)


def test_c5_sh_degree_3_equals_the_sh1_run(dev, c5_cloud):
    """The DEG = 3 instantiations at 20 M splats (bench.py times S3 at SH degree 3: 192-byte v_sh rows on the
    streaming-store path, `sh` byte offsets up to 4.03e9, the [N][12] staging array of the cull kernel).  The f64
    arbiter at SH 3 would hold eight [N,16,3] f64 arrays; instead the same cloud is run with its SH rows padded to
    degree 3 by ZERO bands 2 and 3: the colours are the same bits (col + 0 = col, project_visible.wgsl:51-147), so in
    deterministic mode the image, every aux array, v_means / v_scales / v_quats / v_opac / v_xy and the first four v_sh
    rows must EQUAL the SH-1 run bit for bit (which the test above holds to the oracle), and the twelve new rows must
    be Y_k(dir) x v_rgb with the oracle's basis (gather_grads.wgsl:186-222) — checked on the last 1 000 000 global ids."""
    import torch

    import brush_amd

    n = c5_cloud["means"].shape[0]
    if not C5_STATE:  # run alone: produce the SH-1 state first
        test_c5_scale_20m_splats_4k(dev, c5_cloud)
    sh3 = np.zeros((n, 16, 3), np.float32)
    sh3[:, :4] = c5_cloud["sh"]
    params = {k: _t(c5_cloud[k], dev, grad=True) for k in ("means", "log_scales", "quats", "raw_opac")}
    params["sh"] = _t(sh3, dev, grad=True)
    del sh3
    xy = torch.zeros((n, 2), device=dev, requires_grad=True)
    out, aux = brush_amd.render_splats(_camera(3840, 2160), (3840, 2160), params["means"], xy, params["log_scales"],
                                       params["quats"], params["sh"], params["raw_opac"], False, 24_000_000,
                                       deterministic=True)
    rng = np.random.default_rng(7)  # the upstream gradient _run_pair used
    v_out = (rng.standard_normal((2160, 3840, 4)).astype(np.float32)) / np.float32(2160 * 3840)
    out.backward(_t(v_out, dev))
    torch.cuda.synchronize()
    ref = C5_STATE
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), ref["out"].view(np.uint32))
    for name in ("num_visible", "num_intersections", "final_index", "cum_tiles_hit", "tile_bins", "global_from_compact_gid",
                 "compact_from_global_gid", "projected_splats", "overflow"):
        assert torch.equal(getattr(aux, name), getattr(ref["aux"], name)), name
    I = aux.read_num_intersections()
    assert torch.equal(aux.compact_gid_from_isect[:I], ref["aux"].compact_gid_from_isect[:I])
    got = dict(v_means=params["means"].grad, v_scales=params["log_scales"].grad, v_quats=params["quats"].grad,
               v_opac=params["raw_opac"].grad, v_xy=xy.grad)
    for name, g in got.items():
        assert torch.equal(g, ref["grads"][name]), name
    v_sh = params["sh"].grad
    assert torch.equal(v_sh[:, :4], ref["grads"]["v_sh"]), "bands 0-1 of v_sh differ from the SH-1 run"
    # bands 2-3 on the last 1 000 000 global ids: v_sh[g, k] = Y_k(dir_g) * v_rgb_g, with v_rgb_g = v_sh[g, 0] / Y_0
    m = 1_000_000
    u3 = dict(ref["u"])
    u3["sh_degree"] = 3
    Y = O.sh_basis_for_means(u3, c5_cloud["means"][n - m:])                       # [m, 16] f32, the oracle's basis
    tail = v_sh[n - m:].detach().cpu().numpy().astype(np.float64)                 # [m, 16, 3]
    v_rgb = tail[:, 0, :] / np.float64(Y[0, 0])
    want = Y.astype(np.float64)[:, :, None] * v_rgb[:, None, :]
    vis = np.abs(tail[:, 0, :]).max(axis=1) > 0
    assert vis.sum() > 1000, int(vis.sum())  # (most visible splats of this frame sit behind saturated pixels)
    # one rounding in v_rgb * Y_0, one in Y_k * v_rgb; the basis comes from the same expression tree without contraction,
    # an ulp of the direction (a polynomial that passes through zero) is covered by the term in |v_rgb|
    tol = 4.0 * EPS32 * np.abs(want) + 16.0 * EPS32 * np.abs(v_rgb)[:, None, :] + 1e-45
    assert (np.abs(tail - want) <= tol).all(), float((np.abs(tail - want) / (np.abs(want) + 1e-300)).max())
    assert not tail[~vis].any()
    # and the rows off the visible set are exact zeros everywhere
    gfc = aux.global_from_compact_gid[:aux.read_num_visible()].long()
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    mask[gfc] = False
    assert not bool(v_sh[mask].any())
    C5_STATE.clear()


def test_headline_size_properties(dev):
    """1 M splats @1080p (BASELINE.json metric): structural invariants, run-to-run bit
    reproducibility of the forward, linearity of the backward in v_out."""
    import torch

    import brush_amd

    n, w, h = 1 << 20, 1920, 1080
    cloud = H.synthetic_cloud(n, 0, seed=4)
    p = {k: _t(cloud[k], dev) for k in cloud}

    def run(scale):
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        xy = torch.zeros((n, 2), device=dev, requires_grad=True)
        out, aux = brush_amd.render_splats(_camera(w, h), (w, h), leaves["means"], xy, leaves["log_scales"],
                                           leaves["quats"], leaves["sh"], leaves["raw_opac"], False, 4_000_000)
        (out.mean() * scale).backward()
        return out.detach(), aux, {k: v.grad for k, v in leaves.items()}, xy.grad

    out1, aux1, g1, xy1 = run(1.0)
    out2, aux2, g2, xy2 = run(2.0)
    assert torch.equal(out1, out2) and torch.equal(aux1.final_index, aux2.final_index)
    V, I = aux1.read_num_visible(), aux1.read_num_intersections()
    assert 0 < V < n and 0 < I <= aux1.max_intersects and int(aux1.overflow.item()) == 0
    # visible set is a set of distinct ids, inverse map is consistent
    gfc = aux1.global_from_compact_gid[:V].long()
    assert int(torch.bincount(gfc, minlength=n).max()) == 1
    assert bool((aux1.compact_from_global_gid[gfc] == torch.arange(V, device=dev, dtype=torch.int32)).all())
    assert bool((aux1.global_from_compact_gid[V:] == 0).all())
    # cum_tiles_hit is non-decreasing, its tail equals I
    cum = aux1.cum_tiles_hit.long()
    assert bool((cum[1:] >= cum[:-1]).all()) and int(cum[-1]) == I and int(cum[V - 1]) == I
    # tile bins partition [0, I)
    bins = aux1.tile_bins.long().reshape(-1, 2)
    used = bins[bins[:, 1] > bins[:, 0]]
    assert int((used[:, 1] - used[:, 0]).sum()) == I
    order = torch.argsort(used[:, 0])
    assert bool((used[order][1:, 0] == used[order][:-1, 1]).all())
    # per-tile lists are depth ordered (compact ids ascending within a tile)
    cg = aux1.compact_gid_from_isect[:I].long()
    starts = torch.zeros(I, dtype=torch.bool, device=dev)
    starts[used[:, 0]] = True
    assert bool(((cg[1:] > cg[:-1]) | starts[1:]).all())
    # alpha in [0, 1), image finite
    assert bool(torch.isfinite(out1).all()) and float(out1[..., 3].max()) < 1.0 and float(out1[..., 3].min()) >= 0.0
    # backward is linear in v_out (f32 atomics: tolerance), dense, zero off the visible set
    for k in g1:
        a, b = g1[k].double() * 2.0, g2[k].double()
        scale = float(b.abs().max()) + 1e-30
        assert float((a - b).abs().max()) <= 1e-4 * scale, k
        vis = torch.zeros(n, dtype=torch.bool, device=dev)
        vis[gfc] = True
        assert not bool(g1[k][~vis].any())
    assert float((xy1.double() * 2 - xy2.double()).abs().max()) <= 1e-4 * (float(xy2.abs().max()) + 1e-30)


def test_forward_prezeroes_the_backward_accumulators(dev):
    """Build extension BrushAux::bwd_accum + BRUSH_AUX_ACCUM_ZEROED: the forward's last kernel zeroes the backward's
    accumulator rows, the first backward of that render skips its zero-fill launch, a SECOND backward of the same forward
    zero-fills itself, and a backward that claims pre-zeroed accumulators in another buffer is refused."""
    import ctypes as C

    import torch

    from brush_amd import _lib
    from brush_amd import render as R

    n, w, h, deg = 60_000, 400, 300, 2
    ncoef = (deg + 1) ** 2
    cloud = H.synthetic_cloud(n, deg, seed=21, mean_mult=0.02)
    p = {k: _t(v, dev) for k, v in cloud.items()}
    cam = _camera(w, h)
    v_out = torch.randn((h, w, 4), device=dev) / (h * w)

    def run(expect):
        # the default mode by name: the deterministic mode keeps its sums in pieces and has no rows to pre-zero, so
        # under BRUSH_DETERMINISTIC=1 the environment's default would leave nothing here to test
        out, aux, u = R._forward_impl(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], False,
                                      2_000_000, deterministic=False, expect_backward=expect)
        return out, aux, u

    out0, aux0, u0 = run(False)
    assert aux0.bwd_ws is None
    _, ref = R._backward_impl(u0, aux0, p["means"], p["log_scales"], p["quats"], p["raw_opac"], ncoef, out0, v_out)
    out1, aux1, u1 = run(True)
    assert aux1.bwd_ws is not None and aux1.bwd_ws_zeroed and torch.equal(out0, out1)
    V = aux1.read_num_visible()
    # what the forward left in the accumulator rows: exact zeros (the buffer was poisoned when it was allocated)
    rows = aux1.bwd_ws[:V * 64].view(torch.float32)
    assert V > 1000 and not bool(rows.any())
    _, g1 = R._backward_impl(u1, aux1, p["means"], p["log_scales"], p["quats"], p["raw_opac"], ncoef, out1, v_out)
    assert not aux1.bwd_ws_zeroed
    _, g2 = R._backward_impl(u1, aux1, p["means"], p["log_scales"], p["quats"], p["raw_opac"], ncoef, out1, v_out)
    scale = float(ref.abs().max())
    assert scale > 0
    for g in (g1, g2):  # float atomics: two runs differ in the last bits
        assert float((g - ref).abs().max()) <= 1e-4 * scale
    # the flag with a workspace that is not the one the forward zeroed: refused
    out2, aux2, u2 = run(True)
    s = aux2._as_struct()
    s.flags |= _lib.AUX_ACCUM_ZEROED
    other = torch.empty_like(aux2.bwd_ws)
    blk = torch.zeros(R.grad_block_layout(n, ncoef)[1], device=dev)
    lay, _ = R.grad_block_layout(n, ncoef)
    ptr = lambda name: blk.data_ptr() + 4 * lay[name][0]
    rc = _lib.lib().brush_render_backward(C.byref(u2), C.byref(s), p["means"].data_ptr(), p["log_scales"].data_ptr(),
                                          p["quats"].data_ptr(), p["raw_opac"].data_ptr(), n, out2.data_ptr(),
                                          v_out.data_ptr(), ptr("v_means"), ptr("v_xy"), ptr("v_scales"), ptr("v_quats"),
                                          ptr("v_sh"), ptr("v_opac"), other.data_ptr(), other.numel(),
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == -1  # BRUSH_ERR_INVALID_ARG


def test_rejects_bad_shapes(dev):
    import torch

    import brush_amd

    n = 4
    ok = dict(means=torch.zeros((n, 3), device=dev), log_scales=torch.zeros((n, 3), device=dev),
              quats=torch.zeros((n, 4), device=dev), sh=torch.zeros((n, 1, 3), device=dev),
              raw=torch.zeros((n,), device=dev))
    cam = _camera(32, 32)
    with pytest.raises(AssertionError):  # DimCheck (render.rs:74-79)
        brush_amd.render_splats(cam, (32, 32), ok["means"], None, torch.zeros((n, 2), device=dev), ok["quats"],
                                ok["sh"], ok["raw"])
    with pytest.raises(ValueError):  # render.rs:44-52
        brush_amd.render_splats(cam, (32, 32), ok["means"], None, ok["log_scales"], ok["quats"],
                                torch.zeros((n, 5, 3), device=dev), ok["raw"])


def test_degenerate_parameters_stay_in_bounds(dev):
    """NaN / inf / zero / huge parameters (the reference runs its kernels unchecked,
    crates/brush-kernel `execute_unchecked`): every index in this build is clamped or capacity
    checked, so the op must complete with sane counts and leave healthy splats' pixels finite."""
    import torch

    import brush_amd

    n, w, h = 3000, 160, 96
    cloud = H.synthetic_cloud(n, 1, seed=13, mean_mult=0.002)
    bad = np.arange(0, 200)
    cloud["means"][bad[0:20]] = np.nan
    cloud["means"][bad[20:40]] = np.inf
    cloud["means"][bad[40:60], 2] = -8.0 + 0.0100001          # grazing the near cull plane
    cloud["log_scales"][bad[60:80]] = 80.0                     # exp overflows to inf
    cloud["log_scales"][bad[80:100]] = -120.0                  # exp underflows to 0
    cloud["log_scales"][bad[100:110]] = np.nan
    cloud["quats"][bad[110:130]] = 0.0
    cloud["quats"][bad[130:140]] = np.nan
    cloud["raw_opac"][bad[140:160]] = 1e30
    cloud["raw_opac"][bad[160:170]] = -1e30
    cloud["raw_opac"][bad[170:180]] = np.nan
    cloud["sh"][bad[180:200]] = np.inf
    p = {k: _t(v, dev, grad=True) for k, v in cloud.items()}
    xy = torch.zeros((n, 2), device=dev, requires_grad=True)
    out, aux = brush_amd.render_splats(_camera(w, h), (w, h), p["means"], xy, p["log_scales"], p["quats"], p["sh"],
                                       p["raw_opac"], False, 200_000)
    out.nan_to_num().sum().backward()
    torch.cuda.synchronize()
    V, I = aux.read_num_visible(), aux.read_num_intersections()
    assert 0 < V <= n and 0 < I <= aux.max_intersects
    gfc = aux.global_from_compact_gid[:V].long()
    assert int(gfc.max()) < n and int(torch.bincount(gfc, minlength=n).max()) == 1
    bins = aux.tile_bins.long()
    assert int(bins.max()) <= I and bool((bins[..., 1] >= bins[..., 0]).all())
    assert int(aux.compact_gid_from_isect[:I].max()) < V
    for g in (p["means"].grad, p["sh"].grad, xy.grad):
        assert g is not None and g.shape[0] == n
    # the same scene without the poisoned splats renders finite
    keep = np.arange(200, n)
    q = {k: _t(v[keep], dev) for k, v in cloud.items()}
    clean, _ = brush_amd.render_splats(_camera(w, h), (w, h), q["means"], None, q["log_scales"], q["quats"], q["sh"],
                                       q["raw_opac"], False, 200_000)
    assert bool(torch.isfinite(clean).all())


def test_rgba8_row_pitch_matches_padded_u32(dev):
    """the pitched RGBA8 output equals the reference's padding of the packed image
    into a zero [h, ceil(w/64)*64] tensor (burn_texture.rs:17-26), bit for bit."""
    import torch

    import brush_amd

    for (w, h) in ((123, 82), (128, 40), (1000, 37)):
        cloud = H.synthetic_cloud(3000, 1, seed=21, mean_mult=0.002)
        p = {k: _t(v, dev) for k, v in cloud.items()}
        cam = _camera(w, h)
        tight, _ = brush_amd.render_splats(cam, (w, h), p["means"], None, p["log_scales"], p["quats"], p["sh"],
                                           p["raw_opac"], render_u32_buffer=True)
        pitch = brush_amd.rgba8_row_pitch(w)
        assert pitch % 64 == 0 and 0 <= pitch - w < 64
        padded, aux = brush_amd.render_rgba8(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"])
        assert tuple(padded.shape) == (h, pitch, 1)
        want = torch.zeros((h, pitch, 1), dtype=torch.int32, device=dev)
        want[:, :w] = tight
        assert torch.equal(padded, want)
        assert int(tight.abs().max()) != 0 and aux.read_num_visible() > 0
    with pytest.raises(ValueError):
        brush_amd.render._forward_impl(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], True, None,
                                       row_pitch=w - 1)


@pytest.mark.parametrize("deg", [3, 0, 2])  # v_sh rows of whole cache lines (3) and the scalar store paths (0, 2)
def test_view_records_round_trip(dev, deg):
    """brush_amd.dist: the 64-byte records of one view (brush_render_backward_records) reduced over that single view
    (brush_reduce_view_records) reproduce the op's dense gradients bit for bit: same projection VJP, same SH basis,
    0 + x = x.  (The multi-GPU exchange all-gathers these records instead of all-reducing 52+12C bytes/splat.)"""
    import torch

    import brush_amd
    from brush_amd import dist as BD
    from brush_amd import render as R

    n, w, h = 50000, 320, 240
    C = (deg + 1) ** 2
    cloud = H.synthetic_cloud(n, deg, seed=6, mean_mult=0.01)
    p = {k: _t(v, dev) for k, v in cloud.items()}
    out, aux, u = R._forward_impl(_camera(w, h), (w, h), p["means"], p["log_scales"], p["quats"], p["sh"],
                                  p["raw_opac"], False, 2_000_000)
    v_out = torch.randn((h, w, 4), device=dev) / (h * w)
    g, block = R._backward_impl(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], C, out, v_out)
    V = aux.read_num_visible()
    xchg = BD.ViewExchange(n, C, dev, packed=True)
    xchg.begin(aux)
    xchg.backward_records(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], out, v_out)
    recs = xchg.gather()  # packed form: a list with one [V, 16] view of the flat buffer per view
    assert len(recs) == 1 and recs[0].shape[0] == V and xchg.counts() == [V]
    recs = recs[0].unsqueeze(0)  # [1, V, 16] view of the same memory
    want = BD.records_from_dense_torch(g, aux, n, (w, h), V)
    assert torch.equal(recs[0, :V, 0].contiguous().view(torch.int32), want[:V, 0].contiguous().view(torch.int32))
    # everything but v_rgb is the same arithmetic on the same compact sums (float atomics: two backward runs differ
    # in the last bits), v_rgb differs from v_sh0 / Y0 by one rounding
    assert float((recs[0, :V, 1:] - want[:V, 1:]).abs().max()) <= 1e-4 * float(want[:V, 1:].abs().max())
    grads, red = xchg.reduce_dense(p["means"])
    # reduce the records the torch way too and compare: the HIP reduction is exactly that sum
    ref = BD.reduce_view_records_torch(recs, xchg.metas[:, 0], xchg.metas[:, 1:4].contiguous().view(torch.float32),
                                       p["means"], n, C)
    for name in ("v_means", "v_scales", "v_quats", "v_opac"):
        assert torch.equal(grads[name], ref[name]), name
    assert float((grads["v_sh"] - ref["v_sh"]).abs().max()) <= 2e-6 * float(ref["v_sh"].abs().max())
    # against the dense backward of the op (second run of the atomics: tolerance)
    layout, _ = R.grad_block_layout(n, C)
    for name in ("v_means", "v_scales", "v_quats", "v_opac", "v_sh"):
        off, sz = layout[name]
        a, b = red[off:off + sz].double(), block[off:off + sz].double()
        assert float((a - b).abs().max()) <= 1e-4 * (float(b.abs().max()) + 1e-30), name
    vis = torch.zeros(n, dtype=torch.bool, device=dev)
    vis[aux.global_from_compact_gid[:V].long()] = True
    assert not bool(grads["v_sh"][~vis].any()) and not bool(grads["v_means"][~vis].any())
    # a stale index (left by this call) must not leak into a later reduction of other records
    dropped = recs[0, :V // 2, 0].contiguous().view(torch.int32).long().clone()  # `recs` is a view of xchg.gathered
    recs[0, :V // 2, 0] = torch.tensor(n + 5, dtype=torch.int32, device=dev).view(torch.float32)
    grads2, _ = xchg.reduce_dense(p["means"])
    assert not bool(grads2["v_means"][dropped].any())  # records whose gid is out of range are ignored, entries re-validated


@pytest.mark.parametrize("packed", [True, False])
def test_view_records_many_views(dev, packed):
    """Five views of one cloud on one GPU, their records laid out as the all-gather would leave them (packed: view after
    view at exact sizes with row offsets; padded: every view at the stride of the largest): the HIP reduction
    (dense form) adds a splat's records in view order exactly like the torch restatement (bit for bit for the per-splat
    vectors, v_sh to rounding), twice in a row on the same index buffer (entries consumed by the first call are gone,
    the second rebuilds them), and splats no view sees get exact zeros."""
    import torch

    import brush_amd
    from brush_amd import dist as BD
    from brush_amd import render as R

    n, w, h, deg, W = 60000, 320, 240, 3, 5
    C = (deg + 1) ** 2
    cloud = H.synthetic_cloud(n, deg, seed=12, mean_mult=0.01)
    p = {k: _t(v, dev) for k, v in cloud.items()}
    v_out = torch.randn((h, w, 4), device=dev) / (h * w)
    base = H.reference_test_camera(w, h)
    views, seen = [], torch.zeros(n, dtype=torch.bool, device=dev)
    for r in range(W):
        ang = 0.3 * r
        rot = [0.0, math.sin(ang / 2), 0.0, math.cos(ang / 2)]
        pos = [-4.0 * math.sin(ang), 0.0, -4.0 * math.cos(ang)]
        cam = brush_amd.Camera(pos, rot, base["fov_x"], base["fov_y"], base["center_uv"])
        out, aux, u = R._forward_impl(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], False,
                                      2_000_000)
        x = BD.ViewExchange(n, C, dev, packed=True)
        x.begin(aux)
        x.backward_records(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], out, v_out)
        recs = x.gather()
        V = aux.read_num_visible()
        assert V > 500 and recs[0].shape[0] == V
        seen[aux.global_from_compact_gid[:V].long()] = True
        views.append((recs[0].clone(), x.metas.clone()))
    rows = max(v[0].shape[0] for v in views)
    x = BD.ViewExchange(n, C, dev, packed=packed)
    x.world = W
    x.metas = torch.cat([v[1] for v in views], 0).contiguous()
    x._ensure_capacity(rows)
    if packed:
        counts = [v[0].shape[0] for v in views]
        offs = [sum(counts[:i]) for i in range(W)]
        x._rows = sum(counts)
        x._offsets_dev = torch.tensor(offs, dtype=torch.int32, device=dev)
        flat = x.gathered[:x._rows * 16].view(-1, 16)
        g = []
        for i, v in enumerate(views):
            flat[offs[i]:offs[i] + counts[i]] = v[0]
            g.append(flat[offs[i]:offs[i] + counts[i]])
    else:
        x._rows = rows
        g = x.gathered[:W * rows * 16].view(W, rows, 16)
        for i, v in enumerate(views):
            g[i, :v[0].shape[0]] = v[0]
    ref = BD.reduce_view_records_torch(g, x.metas[:, 0], x.metas[:, 1:4].contiguous().view(torch.float32), p["means"], n, C)
    for rep in range(2):
        grads, _ = x.reduce_dense(p["means"])
        for name in ("v_means", "v_scales", "v_quats", "v_opac"):
            assert torch.equal(grads[name], ref[name]), (name, rep)
        assert float((grads["v_sh"] - ref["v_sh"]).abs().max()) <= 4e-6 * float(ref["v_sh"].abs().max())
        assert not bool(grads["v_sh"][~seen].any()) and not bool(grads["v_quats"][~seen].any())
        assert bool(grads["v_means"][seen].any())


def test_training_steps_reduce_loss(dev):
    """the reference's step (L1 + 0.2*SSIM, five Adam groups, SH lerp) drives
    the op end to end; fitting a render of perturbed parameters must reduce the loss."""
    import torch

    import brush_amd

    torch.manual_seed(0)
    cloud = H.synthetic_cloud(4000, 1, seed=8, mean_mult=0.002)
    w, h = 160, 96
    cam = _camera(w, h)

    def mk(c):
        return brush_amd.Splats(_t(c["means"], dev), _t(c["sh"], dev), _t(c["quats"], dev), _t(c["raw_opac"], dev),
                                _t(c["log_scales"], dev))

    with torch.no_grad():
        target, _ = mk(cloud).render(cam, (w, h))
    pert = dict(cloud)
    rng = np.random.default_rng(1)
    pert["sh"] = cloud["sh"] + rng.normal(0, 0.3, cloud["sh"].shape).astype(np.float32)
    pert["raw_opac"] = cloud["raw_opac"] - 0.5
    splats = mk(pert)
    trainer = brush_amd.SplatTrainer(splats, brush_amd.TrainConfig(warmup_steps=2))
    losses = []
    for _ in range(40):
        loss, pred, aux = trainer.step(splats, cam, target[..., :3].contiguous(), scene_extent=1.0)
        losses.append(float(loss))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] - 0.02, (losses[0], losses[-1])
    assert trainer.iter == 40 and float(trainer.xy_grad_counts.max()) > 0
