"""The optimizer kernels against the float64 references of tests/ref64.py, element by element: brush_adam_step (both
layouts, SH degree 0-4, the quaternion chain rule, times 1 .. 30000, subnormal and overflowing moments),
brush_normalize_quats and brush_lazy_sh_flush (a hand-built deferred-SH state).  Every step is compared with the reference
fed the GPU's own previous state: chained drift is not a kernel property.  Each test records its worst err/tol in
tests/margins.py (sections adam, replay, quats).

The hard ceiling of the Adam allowance (tests/ref64.py: 1e-4 of the step's own terms plus half an ulp of x) has these
exemptions, each a named term, each counted and printed:
- the subnormal term (v' / bc2 < FLT_MIN: v_sqrt_f32 flushes the argument) and the subnormal floors of the moments;
- the quaternion chain rule's error, on quaternion elements with rotation_grad_wrt_normalized: where v_q / s and
  q (v_q . q) / s^3 cancel, its float32 rounding is a large part of the chained gradient, and Adam normalises the step
  by that gradient's own size; for |q| > 4.4e12 the kernel's float32 s^-3 is subnormal and the second term is lost
  (rows at |q| = 1e13 reach it);
- the lerp of the SH-rest coefficients: x (1 - l) + stepped l rounds at the scale of x, so its ceiling is 1e-4 of the
  lerped step's terms plus 3 U |x| (about 1.5 ulp of x) instead of half an ulp."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import helpers as H
from tests import margins
from tests import ref64 as R64

pytestmark = pytest.mark.gpu

LRS = (1.6e-4, 0.01, 0.002, 0.05, 0.004)   # means, log_scales, quats, raw_opac, sh (TrainConfig defaults)
LERP = np.float32(1.0 / 20.0)
B1, B2, EPS = 0.9, 0.999, 1e-15
TIMES = (1, 2, 3, 10, 1000, 30000)
TIMES_LARGE = (1, 10, 30000)   # n = 65540: its float64 passes cost a second each


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _signed_log(rng, shape, lo, hi):
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(lo, hi, size=shape)).astype(np.float32)


def _grads(rng, shape):
    """+0, -0 and signed log-uniform 1e-30 .. 1e3."""
    g = _signed_log(rng, shape, -30, 3)
    c = rng.random(shape)
    g[c < 0.04] = 0.0
    g[(c >= 0.04) & (c < 0.08)] = -0.0
    return g


def _moments(rng, shape, g, rbc2):
    """m signed log-uniform; v chosen so that v' / bc2 lands in [0, FLT_MIN), near eps^2 = 1e-30 (sqrt(v) ~ eps) or
    anywhere up to 1e6; the gradient of the first two classes is made small enough not to lift v' out of its class."""
    m = _signed_log(rng, shape, -20, 2)
    v = (10.0 ** rng.uniform(-20, 6, size=shape)).astype(np.float32)
    c = rng.random(shape)
    sub, near, zero = c < 0.1, (c >= 0.1) & (c < 0.2), (c >= 0.2) & (c < 0.24)
    v[sub] = (10.0 ** rng.uniform(-45, math.log10(R64.FLT_MIN), size=int(sub.sum())) / (B2 * rbc2)).astype(np.float32)
    v[near] = (10.0 ** rng.uniform(-31, -29, size=int(near.sum())) / (B2 * rbc2)).astype(np.float32)
    v[zero] = 0.0
    scale = np.ones(shape)
    scale[sub], scale[near], scale[zero] = 1e-30, 1e-18, 0.0
    g *= scale.astype(np.float32)
    m[sub] = _signed_log(rng, int(sub.sum()), -25, -12)
    m[near] = _signed_log(rng, int(near.sum()), -22, -12)
    return m, v, scale


def _params(rng, n, ncoef):
    x = [_signed_log(rng, (n, 3), -3, 3), rng.standard_normal((n, 3)).astype(np.float32),
         None, rng.standard_normal(n).astype(np.float32), _signed_log(rng, (n, ncoef * 3), -3, 2)]
    q = rng.standard_normal((n, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))  # norms 1e-3 .. 1e3
    x[2] = q.astype(np.float32)
    x[0][rng.random((n, 3)) < 0.02] = 0.0
    if n >= 1000:   # |q| > 4.4e12: the kernel's float32 |q|^-3 is subnormal (the chain rule's lost term)
        x[2][-2:] = (x[2][-2:] / np.linalg.norm(x[2][-2:], axis=1, keepdims=True) * 1e13).astype(np.float32)
    return x


class _Adam:
    """Device buffers of one brush_adam_step problem; `shift`: one array offset by 4 bytes inside a larger allocation
    (reaches the scalar layout with n % 4 == 0)."""

    def __init__(self, dev, n, deg, shift=None):
        import torch

        self.n, self.deg, self.ncoef = n, deg, (deg + 1) ** 2
        self.sizes = [3 * n, 3 * n, 4 * n, n, 3 * self.ncoef * n]
        self.total = sum(self.sizes)
        self.dev = dev
        self.shift = shift
        mk = lambda k, name: torch.zeros(k + (1 if shift == name else 0), device=dev)
        self.x = [mk(k, f"x{i}") for i, k in enumerate(self.sizes)]
        self.g = [mk(k, f"g{i}") for i, k in enumerate(self.sizes)]
        self.m1, self.m2 = mk(self.total, "m1"), mk(self.total, "m2")

    def view(self, t, name):
        return t[1:] if self.shift == name else t

    def xs(self):
        return [self.view(t, f"x{i}") for i, t in enumerate(self.x)]

    def gs(self):
        return [self.view(t, f"g{i}") for i, t in enumerate(self.g)]

    def ms(self):
        return self.view(self.m1, "m1"), self.view(self.m2, "m2")

    def ptr(self, t, name):
        return t.data_ptr() + (4 if self.shift == name else 0)

    def step(self, time, vjp, lrs=LRS):
        import torch

        from brush_amd import _lib

        cfg = _lib.BrushAdamConfig(lrs[0], lrs[1], lrs[2], lrs[3], lrs[4], float(LERP), B1, B2, EPS, time, vjp)
        with torch.cuda.device(self.dev):
            _lib.check(_lib.lib().brush_adam_step(
                C.byref(cfg), self.n, self.deg, *[self.ptr(t, f"x{i}") for i, t in enumerate(self.x)],
                *[self.ptr(t, f"g{i}") for i, t in enumerate(self.g)], self.ptr(self.m1, "m1"), self.ptr(self.m2, "m2"),
                torch.cuda.current_stream().cuda_stream), "brush_adam_step")
        torch.cuda.synchronize()


def _rest_mask(ncoef):
    return np.arange(3 * ncoef) >= 3   # SH coefficients >= 1 take the lerp (train.rs:336-351)


def _check_groups(st, pre, post, time, vjp, mutate=None, enforce=True):
    """Compares the post-step GPU state with adam64 fed the pre-step GPU state; returns the per-group worst ratios and
    the elements priced by the subnormal term.  enforce=False: only measure (negative controls)."""
    n, ncoef = st.n, st.ncoef
    shapes = [(n, 3), (n, 3), (n, 4), (n, 1), (n, 3 * ncoef)]
    off = 0
    out = {}
    nsub = nchain = 0
    for i, shp in enumerate(shapes):
        k = st.sizes[i]
        x0, g = pre["x"][i].reshape(shp), pre["g"][i].reshape(shp)
        m0, v0 = pre["m1"][off:off + k].reshape(shp), pre["m2"][off:off + k].reshape(shp)
        r = R64.adam64(x0, g, m0, v0, lr=LRS[i], beta1=B1, beta2=B2, eps=EPS, time=time,
                       lerp=LERP if i == 4 else None, rest=_rest_mask(ncoef) if i == 4 else None,
                       quat_vjp=bool(vjp) and i == 2, mutate=mutate)
        x1 = post["x"][i].reshape(shp)
        m1, v1 = post["m1"][off:off + k].reshape(shp), post["m2"][off:off + k].reshape(shp)
        wx, ix, bad_x = R64.gate(x1, r["x"], r["tol"])
        wm, _, bad_m = R64.gate(m1, r["m"], r["tol_m"])
        wv, _, bad_v = R64.gate(v1, r["v"], r["tol_v"])
        out[i] = dict(x=wx, m=wm, v=wv, bad=bad_x + bad_m + bad_v, at=ix, tol=float(r["tol"].flat[ix]),
                      parts={p: float(np.broadcast_to(t, r["tol"].shape).flat[ix]) for p, t in r["parts"].items()})
        nsub += int(r["sub"].sum())
        nchain += int(r["chain"].sum())
        if enforce:
            if bad_x or bad_m or bad_v:   # the first failing element's inputs and results, for the report
                for name, got, want, tol in (("x", x1, r["x"], r["tol"]), ("m", m1, r["m"], r["tol_m"]),
                                             ("v", v1, r["v"], r["tol_v"])):
                    e = np.argwhere(np.abs(got - want) > np.broadcast_to(tol, want.shape))
                    if len(e):
                        j = tuple(e[0])
                        out[i]["first_bad"] = dict(q=name, at=j, got=float(got[j]), want=float(want[j]),
                                                   tol=float(np.broadcast_to(tol, want.shape)[j]), x=x0[j[0]].tolist(),
                                                   g=g[j[0]].tolist(), m=float(m0[j]), v=float(v0[j]))
                        break
            assert bad_x == 0 and bad_m == 0 and bad_v == 0, (i, time, out[i])
            # hard ceiling: the allowance stays within 1e-4 of the step's own terms (+ half an ulp of x) wherever no
            # subnormal term is used; the subnormal floors and the chain rule's cancellation add their own named terms
            over = (r["tol"] > r["ceil"] * (1.0 + 1e-9)) & ~r["sub"]
            assert not over.any(), (i, time, int(over.sum()), float((r["tol"] / r["ceil"])[over].max()))
        off += k
    return out, (nsub, nchain)


def _snapshot(st):
    m1, m2 = st.ms()
    return dict(x=[t.cpu().numpy().copy() for t in st.xs()], g=[t.cpu().numpy().copy() for t in st.gs()],
                m1=m1.cpu().numpy().copy(), m2=m2.cpu().numpy().copy())


def _fill(st, rng, time):
    """Parameters, gradients and pre-filled moments; st.gscale keeps each element's gradient class for later steps."""
    import torch

    n, ncoef = st.n, st.ncoef
    rbc2 = 1.0 / (1.0 - float(np.float32(B2)) ** time)
    for t, a in zip(st.xs(), _params(rng, n, ncoef)):
        t.copy_(torch.from_numpy(a.reshape(-1)))
    g = np.concatenate([_grads(rng, (k,)) for k in st.sizes])
    m, v, st.gscale = _moments(rng, (st.total,), g, rbc2)
    _put_grads(st, g)
    m1, m2 = st.ms()
    m1.copy_(torch.from_numpy(m)), m2.copy_(torch.from_numpy(v))


def _put_grads(st, g):
    import torch

    off = 0
    for t, k in zip(st.gs(), st.sizes):
        t.copy_(torch.from_numpy(np.ascontiguousarray(g[off:off + k])))
        off += k


def _new_grads(st, rng):
    """Fresh gradients of the same classes (the subnormal / near-eps^2 elements keep a gradient that leaves v' there)."""
    g = np.concatenate([_grads(rng, (k,)) for k in st.sizes])
    _put_grads(st, (g * st.gscale).astype(np.float32))


CASES = [(n, deg, vjp, None) for n in (1, 3, 4, 5, 1003, 4096) for deg in range(5) for vjp in (0, 1)]
CASES += [(65540, 0, 1, None), (65540, 1, 0, None), (65540, 2, 1, None), (65540, 3, 0, None), (65540, 4, 1, None)]
# n % 4 == 0 with one array 4 bytes off its 16-byte alignment: the scalar layout
CASES += [(4096, 3, 1, "x4"), (4, 4, 0, "m2"), (4096, 4, 1, "g2"), (1024, 1, 0, "x0")]


@pytest.mark.parametrize("n,deg,vjp,shift", CASES)
def test_adam_step_matches_float64(dev, n, deg, vjp, shift):
    st = _Adam(dev, n, deg, shift)
    rng = np.random.default_rng(1000 * n + 10 * deg + vjp)
    _fill(st, rng, TIMES[0])
    worst, where, nsub, nchain = {}, {}, 0, 0
    for time in (TIMES if n < 65540 else TIMES_LARGE):
        pre = _snapshot(st)
        st.step(time, vjp)
        post = _snapshot(st)
        res, (ns, nc) = _check_groups(st, pre, post, time, vjp)
        nsub, nchain = nsub + ns, nchain + nc
        for i, r in res.items():
            for q in ("x", "m", "v"):
                key = f"g{i}.{q}"
                if r[q] > worst.get(key, -1.0):
                    worst[key] = r[q]
                    where[key] = dict(time=time, tol=r["tol"], parts=r["parts"]) if q == "x" else dict(time=time)
        _new_grads(st, rng)
    w = max(worst.values())
    k = max(worst, key=worst.get)
    print(f"adam n={n} deg={deg} vjp={vjp} shift={shift}: worst err/tol {w:.3f} at {k} {where[k]}; "
          f"subnormal-priced elements {nsub}; chain-rule-priced elements {nchain}")
    margins.record("adam", "worst", dict(worst=w, at=k, subnormal_priced=nsub, chain_priced=nchain,
                                         **{kk: vv for kk, vv in where[k].items() if kk != "parts"}))
    margins.check_growth("adam", "worst", w)


def test_adam_step_overflowing_square(dev):
    """|g| > 1.8e19: float32 g^2 overflows, v becomes inf, the step is 0 and x stays as it was (burn's float32 Adam,
    not the float64 value)."""
    import torch

    n = 8
    st = _Adam(dev, n, 0)
    rng = np.random.default_rng(5)
    xs = _params(rng, n, 1)
    for t, a in zip(st.xs(), xs):
        t.copy_(torch.from_numpy(a.reshape(-1)))
    big = np.array([1.9e19, -2e19, 1e25, -3e30, 1e35, -3.3e38, 2.5e19, -1e20], np.float32)
    gs = [np.resize(big, k).astype(np.float32) for k in st.sizes]
    for t, a in zip(st.gs(), gs):
        t.copy_(torch.from_numpy(a))
    m1, m2 = st.ms()
    m1.fill_(0.5), m2.fill_(1.0)
    pre = _snapshot(st)
    st.step(7, 0)
    post = _snapshot(st)
    for i in (0, 1, 2, 3, 4):
        assert np.array_equal(post["x"][i], pre["x"][i]), i
    assert np.all(np.isinf(post["m2"])) and np.all(post["m2"] > 0)
    g = np.concatenate(gs)
    want_m = np.float32(0.5) * np.float32(B1) + g * (np.float32(1.0) - np.float32(B1))
    assert np.array_equal(post["m1"], want_m.astype(np.float32))


def test_sqrt_of_subnormal_second_moment(dev):
    """What v_sqrt_f32 does with a subnormal argument v' / bc2 < FLT_MIN: the step with the root and the step with the
    root flushed to 0 differ by sqrt(v' / bc2) / eps (up to 1.1e-4 relative).  The measured behaviour must be the one
    tests/ref64.py prices (SQRT_FLUSHES_SUBNORMAL)."""
    import torch

    n, time = 16, 1000
    st = _Adam(dev, n, 0)
    rbc2 = 1.0 / (1.0 - float(np.float32(B2)) ** time)
    rbc1 = 1.0 / (1.0 - float(np.float32(B1)) ** time)
    # targets of v' / bc2: subnormal (flush visible), and normal ones as a control
    a_want = np.array([1.1e-38, 8e-39, 5e-39, 2e-39, 1e-39, 5e-40, 1e-40, 3e-41] + [2e-38, 5e-38, 1e-37, 1e-36] * 2)
    for t in st.xs():
        t.zero_()
    for t in st.gs():
        t.zero_()
    m1, m2 = st.ms()
    m1.zero_(), m2.zero_()
    v0 = (a_want / (rbc2 * float(np.float32(B2)))).astype(np.float32)
    m0 = np.full(n * 3, 1e-12, np.float32)
    m1[:3 * n] = torch.from_numpy(m0)
    m2[:3 * n] = torch.from_numpy(np.repeat(v0, 3))
    pre = _snapshot(st)
    st.step(time, 0)
    post = _snapshot(st)
    x = post["x"][0].astype(np.float64).reshape(n, 3)[:, 0]
    vnew = post["m2"][:3 * n].astype(np.float64).reshape(n, 3)[:, 0]
    mnew = post["m1"][:3 * n].astype(np.float64).reshape(n, 3)[:, 0]
    lr = float(np.float32(LRS[0]))
    a = vnew * rbc2
    keep = -lr * mnew * rbc1 / (np.sqrt(a) + EPS)
    flush = -lr * mnew * rbc1 / EPS
    sub = a < R64.FLT_MIN
    rel_gap = np.abs(keep - flush) / np.abs(flush)
    d_keep, d_flush = np.abs(x - keep) / np.abs(flush), np.abs(x - flush) / np.abs(flush)
    flushed = sub & (d_flush < d_keep) & (rel_gap > 1e-6)
    kept = sub & (d_keep < d_flush) & (rel_gap > 1e-6)
    measured = bool(flushed.any())
    print(f"v_sqrt_f32 with a subnormal argument: flushed {int(flushed.sum())}, kept {int(kept.sum())} of "
          f"{int((sub & (rel_gap > 1e-6)).sum())} resolvable elements; relative gap {rel_gap[sub].max():.2e}; "
          f"normal controls |x - keep| / |x| max {d_keep[~sub].max():.2e}")
    assert not (flushed.any() and kept.any()), "mixed behaviour"
    assert (flushed | kept).sum() >= 4, "the probe resolved nothing"
    assert np.all(d_keep[~sub] < 2e-6)   # normal arguments: the root is taken
    margins.record("adam", "sqrt_flushes_subnormal", measured)
    assert measured == R64.SQRT_FLUSHES_SUBNORMAL, measured


@pytest.mark.parametrize("n", [1, 257, 1000, 65539])
def test_normalize_quats_within_few_ulp(dev, n):
    import torch

    from brush_amd import _lib

    rng = np.random.default_rng(n)
    q = rng.standard_normal((n, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * 10.0 ** rng.uniform(-6, 6, size=(n, 1))
    q32 = q.astype(np.float32)
    src = torch.from_numpy(q32).to(dev)
    out = torch.empty_like(src)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_normalize_quats(src.data_ptr(), out.data_ptr(), n,
                                                    torch.cuda.current_stream().cuda_stream), "brush_normalize_quats")
    got = out.cpu().numpy().astype(np.float64)
    q64 = q32.astype(np.float64)
    want = q64 / np.linalg.norm(q64, axis=1, keepdims=True)
    # |q|^2 (4 products, 3 sums), sqrtf and an IEEE division: a few ulp of each component
    tol = 4.0 * R64.spacing32(want)
    w, i, bad = R64.gate(got, want, tol)
    print(f"normalize_quats n={n}: worst err/tol {w:.3f} (tol 4 ulp)")
    margins.record("quats", "worst", w)
    margins.check_growth("quats", "worst", w)
    assert bad == 0, (w, i)


def _lazy_state(dev, n, deg, base, cap, pend, rng, sh=None):
    import torch

    from brush_amd import _lib

    ncoef = (deg + 1) ** 2
    row = 3 * ncoef
    now = base + cap
    tab = np.empty((cap, 4), np.float32)
    assert _lib.lib().brush_lazy_sh_fill_table(B1, B2, LRS[4], float(LERP), base, cap, tab.ctypes.data) == 0
    t0 = (now - pend[np.arange(n) % len(pend)]).astype(np.int32)
    x = sh if sh is not None else rng.standard_normal((n, row)).astype(np.float32)
    m = _signed_log(rng, (n, row), -6, -1)
    v = (10.0 ** rng.uniform(-10, -1, size=(n, row))).astype(np.float32)
    c = rng.random((n, row))
    v[c < 0.05] = (10.0 ** rng.uniform(-44, -38.5, size=int((c < 0.05).sum()))).astype(np.float32)  # subnormal v' / bc2
    m[c < 0.05] = _signed_log(rng, int((c < 0.05).sum()), -20, -17)
    bufs = dict(table=torch.from_numpy(tab).to(dev), sh_time=torch.from_numpy(t0).to(dev),
                m1=torch.from_numpy(m).to(dev), m2=torch.from_numpy(v).to(dev), sh=torch.from_numpy(x).to(dev))
    z = _lib.BrushLazySh()
    z.table, z.base, z.capacity, z.now = bufs["table"].data_ptr(), base, cap, now
    z.sh_time = bufs["sh_time"].data_ptr()
    z.sh_moment1, z.sh_moment2 = bufs["m1"].data_ptr(), bufs["m2"].data_ptr()
    z.beta1, z.beta2, z.epsilon = B1, B2, EPS
    return z, bufs, dict(x=x, m=m, v=v, t0=t0, now=now)


@pytest.mark.parametrize("deg", [1, 3])
def test_lazy_sh_flush_matches_replay64(dev, deg):
    """A hand-built BrushLazySh: per-splat 0, 1, 2, 7, capacity - 1 and capacity pending steps (now - base ==
    capacity, what the host entry points accept).  The flushed coefficients and both moments match replay64, every
    sh_time becomes `now`, and the forward's in-register replay renders the flushed coefficients' colours."""
    import torch

    import brush_amd
    from brush_amd import _lib
    from brush_amd import render as R

    n, base, cap = 4000, 37, 9
    pend = np.array([0, 1, 2, 7, cap - 1, cap])
    cloud = H.synthetic_cloud(n, deg, seed=31, mean_mult=0.0005)
    cloud["log_scales"] = cloud["log_scales"] - 3.0
    rng = np.random.default_rng(deg)
    sh0 = np.ascontiguousarray(cloud["sh"].reshape(n, -1), np.float32)
    z, bufs, host = _lazy_state(dev, n, deg, base, cap, pend, rng, sh=sh0)
    ncoef = (deg + 1) ** 2
    w, h = 128, 80
    c = H.reference_test_camera(w, h)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    geo = [t(cloud["means"]), t(cloud["log_scales"]), t(cloud["quats"])]
    sh_dev = bufs["sh"].view(n, ncoef, 3)
    img_lazy, _, _ = R._forward_impl(cam, (w, h), geo[0], geo[1], geo[2], sh_dev, t(cloud["raw_opac"]), False, None,
                                     deterministic=True, expect_backward=False, lazy_sh=z)
    img_lazy = img_lazy.clone()
    assert torch.equal(bufs["sh"].cpu(), torch.from_numpy(sh0)), "the forward must not write the coefficients"
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_lazy_sh_flush(C.byref(z), bufs["sh"].data_ptr(), n, deg,
                                                  torch.cuda.current_stream().cuda_stream), "brush_lazy_sh_flush")
    torch.cuda.synchronize()
    r = R64.replay64(host["x"], host["m"], host["v"], host["t0"], host["now"], lr=LRS[4], beta1=B1, beta2=B2, eps=EPS,
                     lerp=LERP, rest=_rest_mask(ncoef))
    got_x, got_m, got_v = (bufs[k].cpu().numpy() for k in ("sh", "m1", "m2"))
    wx, ix, bx = R64.gate(got_x, r["x"], r["tol"])
    wm, _, bm = R64.gate(got_m, r["m"], r["tol_m"])
    wv, _, bv = R64.gate(got_v, r["v"], r["tol_v"])
    steps = r["steps"][:, 0]
    assert sorted(set(steps.tolist())) == sorted(set(pend.tolist()))
    print(f"lazy flush deg={deg}: worst err/tol x {wx:.3f} (at {int(r['steps'].flat[ix])} pending steps, tol "
          f"{float(r['tol'].flat[ix]):.3e}) m {wm:.3f} v {wv:.3f}; subnormal-priced elements {int(r['sub'].sum())}")
    assert bx == 0 and bm == 0 and bv == 0, (wx, wm, wv)
    assert np.array_equal(got_x[steps == 0], host["x"][steps == 0])   # nothing pending: untouched
    assert bool((bufs["sh_time"] == host["now"]).all())
    w_all = max(wx, wm, wv)
    margins.record("replay", "worst", w_all)
    margins.check_growth("replay", "worst", w_all)
    img_flushed, _, _ = R._forward_impl(cam, (w, h), geo[0], geo[1], geo[2], sh_dev, t(cloud["raw_opac"]), False,
                                        None, deterministic=True, expect_backward=False)
    assert torch.equal(img_lazy, img_flushed)


def test_adam_gate_rejects_wrong_references(dev):
    """Negative controls: the same GPU step compared with a reference mutated in one way must fail the gate."""
    n, deg, vjp = 1024, 3, 1
    st = _Adam(dev, n, deg)
    rng = np.random.default_rng(77)
    _fill(st, rng, 1)
    st.step(1, vjp)
    _new_grads(st, rng)
    failed = {}
    for time in (2, 1000):
        pre = _snapshot(st)
        st.step(time, vjp)
        post = _snapshot(st)
        ok, _ = _check_groups(st, pre, post, time, vjp)   # the true reference passes
        for mut in ("bc_tm1", "eps_in_sqrt", "lerp_coef0", "no_lerp_coef3", "abs_g", "no_quat_chain"):
            res, _ = _check_groups(st, pre, post, time, vjp, mutate=mut, enforce=False)
            failed.setdefault(mut, []).append(sum(r["bad"] for r in res.values()))
        _new_grads(st, rng)
    print("adam negative controls (failing elements at t = 2, 1000):", failed)
    for mut, bad in failed.items():
        assert max(bad) > 0, mut
