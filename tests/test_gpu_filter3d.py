"""The 3D smoothing filter on the GPU: brush_filter3d_rates / _apply / _backward against the float64 statement of
tests/filter3d_ref64.py, their composition with the renderer and the trainer, the training loop under
TrainConfig.filter3d, and the zoom-in the feature exists for.

The worst figures every gate met are written to profiles/filter3d_margins.json (as profiles/mcmc_margins.json is for the
MCMC gates)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import filter3d_ref64 as F
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = F.U
COUNTS = [1, 63, 64, 257, 1000]
# View counts around the LDS chunk of brush_filter3d_rates (C = 64 records): 0, 1, C - 1, C, C + 1, 2 C + 3.
CHUNK = 64
VIEW_COUNTS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
EDGE = 1e-3          # every (splat, view) pair stays this far (relative) from each validity edge
DIRECTED = 2e-3      # the directed splats sit this far inside / outside each edge of view 0
MARGINS = {}

# The gate of the rates.  With p.z = fl(fl(fl(fl(m2 x) + fl(m6 y)) + fl(m10 z)) + m14) the first product goes through its
# own rounding and three additions, so to first order |p.z - exact| <= 4 U sum|terms| (sum|terms| = |m2 x| + |m6 y| +
# |m10 z| + |m14|), i.e. 4 sum|terms| / |p.z| ulps of relative error; nu = fl(fx / p.z) adds 1 U.  max over views is
# 1-Lipschitz in the sup norm, so |nu_gpu - nu_ref| <= max over the valid views of those bounds (ref64.rates64's
# nu_bound).  f = fl(sd / nu) with sd = fl(sqrt(variance)) adds 2 U, and 1 U covers the second-order terms:
#     |f_gpu - f_ref| / f_ref <= max_v nu_bound[i, v] / nu_i + 3 U.
# An unseen splat takes max over the seen ones of f, again 1-Lipschitz: the largest absolute bound among the seen.
RATE_EXTRA_U = 3.0

# The budgets of apply / backward, in units of U, det_expf / det_logf at their documented 2 ulp = 4 U (relative for exp,
# of the result for log).  With s2 = exp(2 l) (2 l is exact), f2 = fl(f f), sum = fl(s2 + f2):
#   s2: 4;  f2: 1;  sum: max(4, 1) + 1 = 5;  l' = 0.5 log(sum): absolute 5 U + 4 U |ln sum| = 2.5 U + 4 U |l'| after the
#   exact halving, which is the relative error of exp(l');
#   q = s2 / sum: 4 + 5 + 1 = 10;  g = f2 / sum: 1 + 5 + 1 = 7;  sqrt(q): 5 + 1 = 6;  c: 3 x 6 + 2 = 20;
#   E = exp(-o): 4;  D = fl(fl(1 - c) + E): absolute dD = 20 U c + U (1 - c) + 4 U E + U D, relative r = dD / D;
#   o' = fl(ln c - ln D): absolute do = (20 U + 4 U |ln c|) + (r + 4 U |ln D|) + U |o'|;
#   sigmoid(o') moves by at most p (1 - p) do e^do (the slope p (1 - p) changes by at most e^do over the interval);
#   v_o = fl(v_o' fl(E / D)): relative 4 + 1 + 1 = 6 U plus r / (1 - r);
#   A = fl(v_l' q): 11;  inv = fl(fl(1 + E) / D): 5 + 1 = 6 U plus r / (1 - r);  B = fl(v_o' fl(g inv)): 7 + 6 + 2 = 15 U
#   plus r / (1 - r);  v_l = fl(A + B): 1 more on each.
# Each budget carries 1 U for the second-order terms.
L_EXTRA_U = 2.5 + 1.0


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    if MARGINS:
        path = os.environ.get("BRUSH_FILTER3D_MARGINS") or os.path.join(ROOT, "profiles", "filter3d_margins.json")
        try:
            old = {}
            if os.path.exists(path):
                with open(path) as f:
                    old = json.load(f)
            old.update(MARGINS)
            with open(path, "w") as f:
                json.dump(old, f, indent=1, sort_keys=True)
        except (OSError, ValueError) as e:  # a read-only checkout: never turn a finished run red from here
            print(f"filter3d margins not written: {e!r}")


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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- 1. rates
SIZES = [(64, 48), (96, 80), (128, 72), (50, 50)]
LONE = np.array([0.1, 0.2, 1005.0])     # seen only by the last view
HIDDEN = np.array([0.0, 0.0, 500.0])    # behind every camera


def _views(nv):
    """nv views: cameras on a ring around the origin with different focal lengths and image sizes; from two views on,
    the last one sits far above the scene and looks away from it (it sees LONE and nothing of the cloud)."""
    ring = nv if nv < 2 else nv - 1
    views = []
    for i in range(ring):
        a = 2.0 * math.pi * i / max(ring, 1) + 0.3
        w, h = SIZES[i % 4]
        eye = (4.0 * math.cos(a), 4.0 * math.sin(a), 1.0 + 0.5 * math.sin(3.0 * a))
        views.append((F.look_at_camera(eye, (0.0, 0.0, 0.0), 0.5 + 0.1 * ((i * 7) % 5), w, h), (w, h)))
    if nv >= 2:
        views.append((F.look_at_camera((0.0, 0.0, 1000.0), (0.0, 0.0, 2000.0), 0.5, 80, 60), (80, 60)))
    return views


def _directed(records, rng, near=0.2, margin=0.15):
    """Ten world points just inside / outside each validity edge of view 0, by DIRECTED; the coordinates the edge
    leaves free (the depth, the position along the edge) are drawn from rng."""
    W, fx, fy, cx, cy, w, h = F.unpack_views(records)
    R, t = W[0, :, :3], W[0, :, 3]
    local = [(rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), near * (1.0 + sgn * DIRECTED)) for sgn in (1, -1)]
    for sgn in (1, -1):  # +1: inside
        for lo in (True, False):
            d, a = rng.uniform(2.5, 3.5), rng.uniform(-0.2, 0.2)
            u = (-margin + sgn * DIRECTED) if lo else (1 + margin - sgn * DIRECTED)
            local.append(((u * w[0] - cx[0]) * d / fx[0], a, d))
        for lo in (True, False):
            d, a = rng.uniform(2.5, 3.5), rng.uniform(-0.2, 0.2)
            v = (-margin + sgn * DIRECTED) if lo else (1 + margin - sgn * DIRECTED)
            local.append((a, (v * h[0] - cy[0]) * d / fy[0], d))
    return (np.asarray(local) - t) @ R  # world = R^T (local - t)


_CASES = {}


def _rates_case(n, nv, kind="mixed"):
    """(means f32 [n,3], records f32 [nv,24], reference dict), asserted in float64 to keep every pair EDGE away from
    every validity edge.  kind "hidden": no splat is seen."""
    from brush_amd.filter3d import view_records

    key = (n, nv, kind)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * n + nv)
    records = view_records(_views(nv))

    def draw(k):
        wide = rng.random(k) < 0.5
        return np.where(wide[:, None], rng.uniform(-5.0, 5.0, (k, 3)), rng.uniform(-1.2, 1.2, (k, 3)))

    if kind == "hidden":
        means = HIDDEN + rng.uniform(-1.0, 1.0, (n, 3))
        fixed = n
    else:
        for _ in range(200):  # the directed rows are near view 0's edges by design; they must clear every other view's
            head = [LONE[None]]
            if nv >= 1:
                head.append(_directed(records, rng))
            head.append(HIDDEN + rng.uniform(-1.0, 1.0, (max(n // 8, 1), 3)))
            head = np.concatenate(head)[:n].astype(np.float32)
            if nv == 0 or F.validity64(head, records)[1].min() >= 1.1 * EDGE:
                break
        fixed = head.shape[0]
        means = np.concatenate([head, draw(n - fixed)])
    means = means.astype(np.float32)
    for _ in range(50):  # re-draw the random rows that came too close to an edge
        _, edge = F.validity64(means, records) if nv else (None, np.full((n, 1), np.inf))
        bad = np.nonzero(edge.min(axis=1) < 1.1 * EDGE)[0]
        bad = bad[bad >= fixed]
        if bad.size == 0:
            break
        means[bad] = draw(bad.size).astype(np.float32)
    ref = F.rates64(means, records)
    if nv:
        _, edge = F.validity64(means, records)
        assert edge.min() >= EDGE, (n, nv, kind, float(edge.min()))
    _CASES[key] = (means, records, ref)
    return _CASES[key]


def _rates(dev, means, records, **kw):
    import torch

    from brush_amd import filter3d_rates

    rec = torch.from_numpy(np.ascontiguousarray(records)).to(dev)
    out = filter3d_rates(torch.from_numpy(means).to(dev), rec, **kw)
    torch.cuda.synchronize()
    return _np(out)


def _rate_gate(ref):
    """Absolute bound on |f_gpu - f_ref| per splat, from the derivation above."""
    f, seen = ref["filter"], ref["seen"]
    gate = np.zeros_like(f)
    if seen.any():
        best = ref["nu"].max(axis=1)
        rel = ref["nu_bound"].max(axis=1)[seen] / best[seen] + RATE_EXTRA_U * U
        gate[seen] = f[seen] * rel
        gate[~seen] = gate[seen].max()
    return gate


def test_chunk_size_is_the_one_the_cases_straddle():
    from brush_amd.filter3d import view_chunk

    c = view_chunk()
    assert c == CHUNK, f"the LDS chunk is now {c}: move VIEW_COUNTS so that they straddle it again"
    assert {0, 1, c - 1, c, c + 1, 2 * c + 3} <= set(VIEW_COUNTS)


@pytest.mark.parametrize("nv", VIEW_COUNTS)
@pytest.mark.parametrize("n", COUNTS)
def test_rates_against_ref64(dev, n, nv):
    means, records, ref = _rates_case(n, nv)
    got = _rates(dev, means, records)
    assert got.shape == (n,) and np.isfinite(got).all() and (got >= 0).all()
    if nv == 0 or not ref["seen"].any():
        assert (got == 0).all()
        return
    assert (got > 0).all()
    if n >= 63 and nv >= 2:
        seen = ref["seen"]
        assert (~seen).sum() >= n // 8 and seen.sum() > n // 4
        assert ref["valid"][0].sum() == 1 and ref["valid"][0, -1]      # LONE: the last view of the last chunk only
        assert ref["valid"][1:11, 0].tolist() == [True, False] + [True] * 4 + [False] * 4   # the directed splats
    # unseen splats carry the largest seen length, bit for bit
    if (~ref["seen"]).any():
        assert (_bits(got[~ref["seen"]]) == _bits(got[ref["seen"]].max())).all()
    gate = _rate_gate(ref)
    ratio = float((np.abs(got.astype(np.float64) - ref["filter"]) / gate).max())
    print(f"rates n={n} V={nv}: worst err/gate {ratio:.4f}")
    _worse("rates_worst_err_over_gate", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("n,nv", [(257, CHUNK + 1), (1000, 2 * CHUNK + 3)])
def test_rates_validity_decisions_match_exactly(dev, n, nv):
    """Every (splat, view) decision, read off the kernel one view at a time: a sentinel far down the view's axis is
    seen with the smallest rate of all, so an unseen splat comes back with the sentinel's bits and a seen one with a
    smaller length."""
    import torch

    from brush_amd import filter3d_rates

    means, records, ref = _rates_case(n, nv)
    W, *_ = F.unpack_views(records)
    rec = torch.from_numpy(np.ascontiguousarray(records)).to(dev)
    outs = []
    for v in range(nv):
        R, t = W[v, :, :3], W[v, :, 3]
        sentinel = (np.array([0.0, 0.0, 1.0e4]) - t) @ R
        aug = np.concatenate([means, sentinel[None].astype(np.float32)])
        outs.append(filter3d_rates(torch.from_numpy(aug).to(dev), rec[v:v + 1]))
    got = _np(torch.stack(outs, dim=1))  # [n + 1, nv]
    assert (got[-1] > 0).all()
    valid_gpu = _bits(got[:-1]) != _bits(got[-1])[None, :]
    assert (got[:-1][valid_gpu] < np.broadcast_to(got[-1], valid_gpu.shape)[valid_gpu]).all()
    mism = int((valid_gpu != ref["valid"]).sum())
    print(f"decisions n={n} V={nv}: {int(ref['valid'].sum())} valid of {n * nv} pairs, {mism} mismatches")
    assert mism == 0


def test_rates_no_splat_seen_and_no_view(dev):
    means, records, ref = _rates_case(257, CHUNK + 1, kind="hidden")
    assert not ref["seen"].any()
    assert (_rates(dev, means, records) == 0).all()
    from brush_amd.filter3d import VIEW_WORDS

    assert (_rates(dev, means, np.zeros((0, VIEW_WORDS), np.float32)) == 0).all()
    import torch

    from brush_amd import filter3d_rates

    assert filter3d_rates(torch.zeros((0, 3), device=dev), _views(3)).shape == (0,)
    assert (_np(filter3d_rates(torch.from_numpy(means).to(dev), [])) == 0).all()


def test_rates_fill_pass_over_several_trips_and_a_misaligned_array(dev):
    """The one-workgroup fill pass takes 16 Ki lengths per trip through float4 accesses when the array is 16-byte
    aligned and goes word by word otherwise (and over the tail): 20 011 splats are two trips and a tail of three, and
    the same call into an array that starts 4 bytes off must give the same bits."""
    import torch

    from brush_amd import _lib

    n, nv = 20011, 3
    means, records, ref = _rates_case(n, nv)
    assert (~ref["seen"]).sum() > 1000 and ref["seen"].sum() > 1000
    got = _rates(dev, means, records)
    gate = _rate_gate(ref)
    assert (np.abs(got.astype(np.float64) - ref["filter"]) <= gate).all()
    assert (_bits(got[~ref["seen"]]) == _bits(got[ref["seen"]].max())).all()
    m, rec = torch.from_numpy(means).to(dev), torch.from_numpy(records).to(dev)
    buf = torch.full((n + 8,), -1.0, device=dev)
    out = buf[1:1 + n]
    assert out.data_ptr() % 16 == 4
    _lib.check(_lib.lib().brush_filter3d_rates(m.data_ptr(), n, rec.data_ptr(), nv, 0.2, 0.15, 0.2, out.data_ptr(),
                                               _lib.current_stream(dev)), "brush_filter3d_rates")
    torch.cuda.synchronize()
    assert _bits(_np(out)).tobytes() == _bits(got).tobytes()
    assert float(buf[0]) == -1.0 and bool((buf[1 + n:] == -1.0).all())  # nothing written outside the n lengths


def test_rates_view_order_repeat_and_options(dev):
    from brush_amd import filter3d_rates

    import torch

    n, nv = 1000, 2 * CHUNK + 3
    means, records, ref = _rates_case(n, nv)
    a = _rates(dev, means, records)
    assert _bits(a).tobytes() == _bits(_rates(dev, means, records)).tobytes()
    perm = np.random.default_rng(5).permutation(nv)
    assert _bits(a).tobytes() == _bits(_rates(dev, means, records[perm])).tobytes()
    assert _bits(a).tobytes() == _bits(_rates(dev, means, records[::-1])).tobytes()
    # the views as objects give the records' result; variance scales the lengths, near / margin move decisions
    b = _np(filter3d_rates(torch.from_numpy(means).to(dev), _views(nv)))
    assert _bits(a).tobytes() == _bits(b).tobytes()
    c = _rates(dev, means, records, variance=0.8)
    assert np.allclose(c, 2.0 * a, rtol=4 * U)
    assert (_rates(dev, means, records, variance=0.0) == 0).all()
    far = _rates(dev, means, records, near=3.0, margin=0.0)
    ref_far = F.rates64(means, records, near=3.0, margin=0.0)
    assert ref_far["seen"].sum() < ref["seen"].sum()
    _, edge_far = F.validity64(means, records, near=3.0, margin=0.0)  # the cloud was cleared for the default edges:
    clear = edge_far.min(axis=1) >= EDGE                               # compare the splats that clear these too
    assert clear.sum() > n // 2 and ref_far["seen"][clear].any()
    if (~ref_far["seen"]).any():
        clear &= ref_far["seen"]  # (an unseen splat's length depends on every other splat's decisions)
    assert np.allclose(far[clear], ref_far["filter"][clear], rtol=1e-4)
    with pytest.raises(ValueError):
        filter3d_rates(torch.from_numpy(means).to(dev), _views(2), variance=-1.0)
    with pytest.raises(ValueError):
        filter3d_rates(torch.from_numpy(means).to(dev)[:, :2], _views(2))


# ---------------------------------------------------------------------------- 2. apply / VJP
def _rows(n, seed=0):
    """l in [-12, 2], o in [-8, 12]; by row: f = 0, e^-9, e^1, f >> s, f << s, log-uniform between."""
    rng = np.random.default_rng(77 * n + seed)
    l = rng.uniform(-12.0, 2.0, (n, 3))
    o = rng.uniform(-8.0, 12.0, n)
    f = np.exp(rng.uniform(-9.0, 1.0, n))
    kind = (np.arange(n) + (1 if n < 6 else 0)) % 6
    f[kind == 0] = 0.0
    f[kind == 1] = math.exp(-9.0)
    f[kind == 2] = math.exp(1.0)
    l[kind == 3] = rng.uniform(-12.0, -10.0, (int((kind == 3).sum()), 3))
    f[kind == 3] = math.exp(1.0)
    l[kind == 4] = rng.uniform(1.5, 2.0, (int((kind == 4).sum()), 3))
    f[kind == 4] = math.exp(-9.0)
    if n >= 64:
        o[:12:2], o[1:12:2] = 12.0, -8.0
    v_l = rng.normal(size=(n, 3)) * 1e-3
    v_o = rng.normal(size=n) * 1e-3
    return [np.ascontiguousarray(a, np.float32) for a in (l, o, f, v_l, v_o)]


def _budgets(l, o, f):
    """The derived budgets of the comment at the top, per row, from float64 quantities."""
    l2, o2, c, p = F.apply64(l, o, f)
    E = np.exp(-o.astype(np.float64))
    D = 1.0 - c + E
    dD = (20.0 * c + (1.0 - c) + 4.0 * E + D) * U
    r = dD / D
    do = (20.0 + 4.0 * np.abs(np.log(c)) + 4.0 * np.abs(np.log(D)) + np.abs(o2) + 1.0) * U + r
    return {"l": (L_EXTRA_U + 4.0 * np.abs(l2)) * U, "sig": p * (1.0 - p) * do * np.exp(do), "r": r / (1.0 - r),
            "l2": l2, "o2": o2, "c": c, "p": p, "E": E, "D": D}


def _apply(dev, l, o, f):
    import torch

    from brush_amd import apply_filter3d

    t = [torch.from_numpy(a).to(dev) for a in (l, o, f)]
    out_l, out_o = apply_filter3d(*t)
    torch.cuda.synchronize()
    for a, b in zip((l, o, f), t):
        assert _np(b).tobytes() == a.tobytes()  # the inputs are untouched
    return _np(out_l), _np(out_o)


def _backward(dev, l, o, f, v_l, v_o):
    import torch

    from brush_amd import _lib
    from brush_amd.filter3d import backward_into

    t = [torch.from_numpy(a.copy()).to(dev) for a in (l, o, f, v_l, v_o)]
    backward_into(t[0], t[1], t[2], l.shape[0], t[3], t[4], _lib.current_stream(dev))
    torch.cuda.synchronize()
    return _np(t[3]), _np(t[4])


@pytest.mark.parametrize("n", COUNTS)
def test_apply_against_ref64(dev, n):
    l, o, f, _, _ = _rows(n)
    got_l, got_o = _apply(dev, l, o, f)
    assert got_l.shape == (n, 3) and got_o.shape == (n,)
    assert np.isfinite(got_l).all() and np.isfinite(got_o).all()
    zero = f == 0
    assert got_l[zero].tobytes() == l[zero].tobytes() and got_o[zero].tobytes() == o[zero].tobytes()
    b = _budgets(l, o, f)
    # what the renderer consumes: exp(l') and sigmoid(o')
    err_l = np.abs(np.exp(got_l.astype(np.float64)) / np.exp(b["l2"]) - 1.0) / b["l"]
    err_s = np.abs(F.sigmoid(got_o) - b["p"]) / b["sig"][:]
    nz = ~zero
    if nz.any():
        print(f"apply n={n}: worst err/budget scales {err_l[nz].max():.4f} opacity {err_s[nz].max():.4f}")
        _worse("apply_scale_worst_err_over_budget", err_l[nz].max())
        _worse("apply_opacity_worst_err_over_budget", err_s[nz].max())
        assert err_l[nz].max() <= 1.0 and err_s[nz].max() <= 1.0
    if n >= 64:
        assert zero.sum() >= n // 6 and (b["c"][nz] < 1e-10).any() and (b["c"][nz] > 1.0 - 1e-6).any()


@pytest.mark.parametrize("n", COUNTS)
def test_backward_against_ref64(dev, n):
    l, o, f, v_l, v_o = _rows(n, seed=1)
    got_l, got_o = _backward(dev, l, o, f, v_l, v_o)
    assert np.isfinite(got_l).all() and np.isfinite(got_o).all()
    zero = f == 0
    assert got_l[zero].tobytes() == v_l[zero].tobytes() and got_o[zero].tobytes() == v_o[zero].tobytes()
    b = _budgets(l, o, f)
    want_l, want_o = F.vjp64(l, o, f, v_l, v_o)
    s2 = np.exp(2.0 * l.astype(np.float64))
    tot = s2 + (f.astype(np.float64) ** 2)[:, None]
    A = np.abs(v_l.astype(np.float64) * s2 / tot)
    B = np.abs(v_o.astype(np.float64))[:, None] * ((f.astype(np.float64) ** 2)[:, None] / tot) \
        * ((1.0 + b["E"]) / b["D"])[:, None]
    gate_l = A * 12.0 * U + B * (16.0 * U + b["r"][:, None]) + (A + B) * U
    gate_o = np.abs(want_o) * (7.0 * U + b["r"])
    nz = ~zero
    if nz.any():
        rl = (np.abs(got_l - want_l)[nz] / gate_l[nz]).max()
        ro = (np.abs(got_o - want_o)[nz] / gate_o[nz]).max()
        print(f"backward n={n}: worst err/budget v_scales {rl:.4f} v_opac {ro:.4f}")
        _worse("backward_scales_worst_err_over_budget", rl)
        _worse("backward_opac_worst_err_over_budget", ro)
        assert rl <= 1.0 and ro <= 1.0


def test_underflowing_opacity_factor_is_floored_and_finite(dev):
    from brush_amd.filter3d import MIN_RAW_OPACITY

    n = 130
    rng = np.random.default_rng(9)
    l = rng.uniform(-45.0, -35.0, (n, 3)).astype(np.float32)   # c ~ (e^-40 / e)^3 underflows float32
    l[::2, 1:] = 0.0                                           # one thin axis only: c ~ e^-41, no underflow
    o = rng.uniform(-8.0, 12.0, n).astype(np.float32)
    o[:4] = [200.0, -200.0, 88.0, -88.0]                       # beyond the clamp of the opacity
    f = np.full(n, math.e, np.float32)
    got_l, got_o = _apply(dev, l, o, f)
    assert np.isfinite(got_l).all() and np.isfinite(got_o).all()
    floor = np.float32(MIN_RAW_OPACITY)
    assert (got_o[1::2] == floor).all() and (got_o[6::2] > floor).all()
    assert np.allclose(got_l[1::2], 1.0, atol=1e-6)            # l' = ln f
    v_l = rng.normal(size=(n, 3)).astype(np.float32)
    v_o = rng.normal(size=n).astype(np.float32)
    back_l, back_o = _backward(dev, l, o, f, v_l, v_o)
    assert np.isfinite(back_l).all() and np.isfinite(back_o).all()


def test_apply_filter3d_through_autograd(dev):
    import torch

    from brush_amd import apply_filter3d

    l, o, f, v_l, v_o = _rows(257, seed=2)
    want_l, want_o = _backward(dev, l, o, f, v_l, v_o)
    tl = torch.from_numpy(l).to(dev).requires_grad_(True)
    to = torch.from_numpy(o).to(dev).requires_grad_(True)
    tf = torch.from_numpy(f).to(dev)
    a, b = torch.from_numpy(v_l).to(dev), torch.from_numpy(v_o).to(dev)
    out_l, out_o = apply_filter3d(tl, to, tf)
    assert out_l.requires_grad and out_o.requires_grad
    g_l, g_o = torch.autograd.grad([out_l, out_o], [tl, to], [a, b], retain_graph=True)
    ((out_l * a).sum() + (out_o * b).sum()).backward()
    for got in ((g_l, g_o), (tl.grad, to.grad)):
        assert _np(got[0]).tobytes() == want_l.tobytes() and _np(got[1]).tobytes() == want_o.tobytes()
    assert _np(a).tobytes() == v_l.tobytes() and _np(b).tobytes() == v_o.tobytes()  # autograd's buffers are not ours
    # one output unused: its gradient is a zero
    out_l, out_o = apply_filter3d(tl, to, tf)
    (g_only,) = torch.autograd.grad([out_l], [tl], [a])
    z_l, _ = _backward(dev, l, o, f, v_l, np.zeros_like(v_o))
    assert _np(g_only).tobytes() == z_l.tobytes()
    with pytest.raises(ValueError):
        apply_filter3d(tl, to, tf[:-1])
    with pytest.raises(ValueError):
        apply_filter3d(tl, to, tf.double())


# ---------------------------------------------------------------------------- 3. composition
PARAMS = ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")


def _scene(dev, n=1000, w=96, h=80):
    import torch

    from brush_amd import Splats, filter3d_rates

    cams = [c for _, c in TL._ring_cameras(4, w, h)]
    gts = [torch.from_numpy(TL.E.noise_image(w, h, 3, 50 + i)).to(dev) for i in range(4)]
    splats = Splats.from_random_config(n, 3, (np.full(3, -1.0), np.full(3, 1.0)), np.random.default_rng(3), dev)
    with torch.no_grad():
        splats.log_scales.add_(torch.randn(n, 3, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 0.5 - 1.5)
    filt = filter3d_rates(splats.means.detach(), [(c, (w, h)) for c in cams])
    return cams, gts, splats, filt, (w, h)


def _param_bits(splats, tr):
    return tuple(_np(getattr(splats, k)).tobytes() for k in PARAMS) + (_np(tr.moment1).tobytes(),
                                                                         _np(tr.moment2).tobytes())


def test_baked_render_is_the_render_of_the_applied_parameters(dev, deterministic):
    import torch

    from brush_amd import apply_filter3d, render_splats

    cams, _, splats, filt, size = _scene(dev)
    assert float(filt.min()) > 0
    baked = splats.bake_filter3d(filt)
    assert baked is not splats and baked.lazy_sh_owner is None and baked.num_splats() == splats.num_splats()
    l2, o2 = apply_filter3d(splats.log_scales.detach(), splats.raw_opacity.detach(), filt)
    assert torch.equal(baked.log_scales.detach(), l2) and torch.equal(baked.raw_opacity.detach(), o2)
    assert not torch.equal(l2, splats.log_scales.detach())
    for aa in (False, True):
        with torch.no_grad():
            a, _ = baked.render(cams[0], size, antialiased=aa)
            rot = splats.rotation.detach()
            b, _ = render_splats(cams[0], size, splats.means.detach(), None, l2,
                                 rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True)),
                                 splats.sh_coeffs.detach(), o2, antialiased=aa)
        assert torch.equal(a, b) and float(a[..., 3].max()) > 0.1


def test_first_filtered_step_is_the_hand_composed_step(dev, deterministic):
    """apply -> render_splats (autograd) -> loss -> VJP -> brush_adam_step by hand, against SplatTrainer.step with the
    filter set: the same kernels on the same inputs in deterministic mode, so the same bits."""
    import ctypes as C

    import torch

    from brush_amd import SplatTrainer, TrainConfig, _lib, apply_filter3d, render_splats
    from brush_amd.render import sh_degree_from_coeffs
    from brush_amd.train import l1_ssim_loss

    cams, gts, splats, filt, size = _scene(dev)
    cfg = TrainConfig()
    with torch.no_grad():
        baked_img, _ = splats.bake_filter3d(filt).render(cams[0], size)
    # by hand, on copies
    p = {k: getattr(splats, k).detach().clone().requires_grad_(True) for k in PARAMS}
    l2, o2 = apply_filter3d(p["log_scales"], p["raw_opacity"], filt)
    norm_rot = p["rotation"]  # from_random_config: identity rotations, already unit
    img, _ = render_splats(cams[0], size, p["means"], None, l2, norm_rot, p["sh_coeffs"], o2)
    loss, v_img = l1_ssim_loss(img.detach(), gts[0], cfg.ssim_weight, cfg.ssim_window_size)
    img.backward(v_img)
    n, ncoef = splats.num_splats(), int(splats.sh_coeffs.shape[1])
    m1, m2 = torch.zeros(n * (11 + 3 * ncoef), device=dev), torch.zeros(n * (11 + 3 * ncoef), device=dev)
    adam = _lib.BrushAdamConfig(cfg.lr_mean, cfg.lr_scale, cfg.lr_rotation, cfg.lr_opac, cfg.lr_coeffs_dc,
                                1.0 / cfg.lr_coeffs_sh_scale, 0.9, 0.999, 1e-15, 1, 1, 1.0)
    hand = {k: v.detach().clone() for k, v in p.items()}
    _lib.check(_lib.lib().brush_adam_step(C.byref(adam), n, sh_degree_from_coeffs(ncoef), hand["means"].data_ptr(),
                                          hand["log_scales"].data_ptr(), hand["rotation"].data_ptr(),
                                          hand["raw_opacity"].data_ptr(), hand["sh_coeffs"].data_ptr(),
                                          p["means"].grad.data_ptr(), p["log_scales"].grad.data_ptr(),
                                          p["rotation"].grad.data_ptr(), p["raw_opacity"].grad.data_ptr(),
                                          p["sh_coeffs"].grad.data_ptr(), m1.data_ptr(), m2.data_ptr(),
                                          _lib.current_stream(dev)), "brush_adam_step")
    # the trainer, fused_backward left at its default: the filter takes the separate-call path whatever it says
    tr = SplatTrainer(splats, cfg)
    tr.set_filter3d(filt)
    assert tr.fused_backward and tr.filter3d is not None
    t_loss, pred, _ = tr.step(splats, cams[0], gts[0], 1.0)
    tr.sync(splats)
    torch.cuda.synchronize()
    assert torch.equal(pred, baked_img) and torch.equal(pred, img.detach())
    assert float(t_loss) == float(loss)
    assert tr._lazy is None
    for k in PARAMS:
        assert torch.equal(getattr(splats, k).detach(), hand[k]), k
        assert not torch.equal(hand[k], p[k].detach()), k
    assert torch.equal(tr.moment1, m1) and torch.equal(tr.moment2, m2)
    # and it differs from the unfiltered step
    _, _, other, _, _ = _scene(dev)
    SplatTrainer(other, cfg).step(other, cams[0], gts[0], 1.0)
    assert not torch.equal(other.log_scales.detach(), splats.log_scales.detach())


def test_filter_off_is_the_parent_path_bitwise(dev, deterministic):
    import torch

    from brush_amd import SplatTrainer, TrainConfig

    runs = []
    for cfg in (TrainConfig(warmup_steps=2, refine_every=100),
                TrainConfig(warmup_steps=2, refine_every=100, filter3d=False, filter3d_every=7, filter3d_variance=0.5)):
        cams, gts, splats, _, _ = _scene(dev)
        tr = SplatTrainer(splats, cfg)
        assert tr.filter3d is None
        out = []
        for i in range(6):
            tr.step(splats, cams[i % 4], gts[i % 4], 1.0)
        assert tr._lazy is not None  # the default fused, deferred path
        tr.sync(splats)
        torch.cuda.synchronize()
        runs.append(_param_bits(splats, tr) + (_np(tr.grad_2d_accum).tobytes(),))
    assert runs[0] == runs[1]


def test_stale_missing_and_combined_filters(dev):
    import torch

    from brush_amd import SplatTrainer, TrainConfig
    from brush_amd.exposure import ExposureTable
    from brush_amd.pose import PoseTable

    cams, gts, splats, filt, (w, h) = _scene(dev)
    tr = SplatTrainer(splats, TrainConfig(filter3d=True))
    with pytest.raises(ValueError, match="set_filter3d"):
        tr.step(splats, cams[0], gts[0], 1.0)
    tr.set_filter3d(filt[:-1].contiguous())
    with pytest.raises(ValueError, match="stale 3D filter"):
        tr.step(splats, cams[0], gts[0], 1.0)
    tr.set_filter3d(filt)
    with pytest.raises(ValueError, match="single-view"):
        tr.step(splats, cams[0], gts[0], 1.0, exchange=object())
    with pytest.raises(ValueError):
        tr.set_filter3d(filt.double())
    assert tr.iter == 0
    # a refinement changes the count: the next step refuses the old filter
    tr = SplatTrainer(splats, TrainConfig(filter3d=True, warmup_steps=0, refine_every=3, densify_grad_thresh=1e-7))
    tr.set_filter3d(filt)
    n0 = splats.num_splats()
    for i in range(2):  # iteration 1 refines
        tr.step(splats, cams[i % 4], gts[i % 4], 1.0)
    assert tr.last_refine is not None and splats.num_splats() != n0
    with pytest.raises(ValueError, match="stale 3D filter"):
        tr.step(splats, cams[0], gts[0], 1.0)
    # with antialiased + background + pose + exposure, and with depth supervision
    for kind in ("views", "depth"):
        cams, gts, splats, filt, (w, h) = _scene(dev)
        if kind == "views":
            tr = SplatTrainer(splats, TrainConfig(filter3d=True, antialiased=True, background="white"))
            kw = dict(poses=PoseTable(4, 1e-3, 5e-4, 1e-6), exposures=ExposureTable(4, dev, 1e-2, 1e-6),
                      background="white", gt_mask=(torch.rand((h, w), device=dev) > 0.2).to(torch.uint8))
        else:
            tr = SplatTrainer(splats, TrainConfig(filter3d=True, depth_weight=0.1))
            kw = dict(gt_depth=torch.full((h, w), 4.0, device=dev))
        tr.set_filter3d(filt)
        before = splats.log_scales.detach().clone()
        for i in range(3):
            extra = dict(kw, view_index=i % 4) if kind == "views" else kw
            loss, pred, _ = tr.step(splats, cams[i % 4], gts[i % 4], 1.0, **extra)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(pred).all())
        for k in PARAMS:
            assert bool(torch.isfinite(getattr(splats, k)).all()), (kind, k)
        assert not torch.equal(before, splats.log_scales.detach())


# ---------------------------------------------------------------------------- 4. training loop
@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    return TL._write_scene(str(tmp_path_factory.mktemp("filter3d_scene")), dev, w=64, h=64, n_train=8, n_val=2)


def test_loop_refreshes_on_schedule_and_returns_the_baked_splats(dev, scene_dir, monkeypatch):
    import torch

    from brush_amd import TrainConfig
    from brush_amd.eval import eval_stats
    from brush_amd.train_loop import TrainLoop, load_dataset

    data, _ = load_dataset(scene_dir)
    cfg = TrainConfig(filter3d=True, filter3d_every=20, warmup_steps=10, refine_every=25, contribution_prune_at=(44,),
                      contribution_prune_min=0.0)
    loop = TrainLoop(data, cfg, steps=60, init_count=1500, sh_degree=3, seed=3)
    assert loop.log.filter3d and loop.trainer.filter3d is None
    real_step, used = loop.trainer.step, []

    def step(splats, *a, **kw):
        f = loop.trainer.filter3d
        assert f is not None and f.shape[0] == splats.num_splats()  # the filter always has the current length
        used.append((loop.done, f.data_ptr(), splats.num_splats()))
        return real_step(splats, *a, **kw)

    monkeypatch.setattr(loop.trainer, "step", step)
    changed, n = [], loop.splats.num_splats()
    row0, _ = loop.evaluate()
    for i in range(60):
        loop.step()
        if loop.splats.num_splats() != n:
            changed.append(i)
            n = loop.splats.num_splats()
    assert changed and len(used) == 60 and loop.trainer.iter == 60
    assert any(i % 25 == 1 for i in changed)  # a refinement inside the run
    # before the first step, every 20 steps, and in front of the step after each count change; the evals at step 0
    # and at the end bake under the filter of that moment and refresh only when the count changed since
    want = sorted({0, 20, 40} | {i + 1 for i in changed if i + 1 < 60})
    got = loop.log.filter3d_refreshes
    assert [s for s in got if s < 60] == want, (got, changed)
    row, _ = loop.evaluate()
    splats, log = loop.finish()
    assert splats is not loop.splats and splats.num_splats() == loop.splats.num_splats() == log.num_splats
    assert loop.trainer.filter3d.shape[0] == splats.num_splats()
    baked = loop.splats.bake_filter3d(loop.trainer.filter3d)
    assert torch.equal(splats.log_scales, baked.log_scales) and torch.equal(splats.raw_opacity, baked.raw_opacity)
    assert not torch.equal(splats.log_scales, loop.splats.log_scales)
    # the returned splats render what the last eval scored
    again = eval_stats(splats, data.eval)
    assert np.float32(again.mean_psnr()).view(np.int32) == np.float32(row.psnr).view(np.int32)
    assert log.filter3d and log.to_json()["filter3d"] is True and log.prunes and log.prunes[0][0] == 44
    assert np.isfinite(log.losses).all()
    first, last = float(np.mean(log.losses[:10])), float(np.mean(log.losses[-10:]))
    print(f"filter3d loop: loss {first:.4f} -> {last:.4f}, psnr {row0.psnr:.2f} -> {row.psnr:.2f}, "
          f"splats {used[0][2]} -> {splats.num_splats()}, refreshes {got}")
    MARGINS["loop"] = {"loss_first10_last10": [first, last], "psnr": [row0.psnr, row.psnr], "refreshes": got}
    assert last < first


def test_loop_steps_do_not_synchronise_refreshes_included(dev, scene_dir):
    import torch

    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop, load_dataset

    data, _ = load_dataset(scene_dir)
    loop = TrainLoop(data, TrainConfig(filter3d=True, filter3d_every=5, warmup_steps=5, refine_every=50), steps=30,
                     init_count=1000, seed=1)
    loop.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the mode sees a readback on this torch build
            loop.losses[0].item()
        for _ in range(20):  # steps 1..20: the refreshes at 5, 10, 15 and 20 are launches only
            loop.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loop.trainer.last_refine is None and loop.done == 21
    assert loop.log.filter3d_refreshes == [0, 5, 10, 15, 20]


def test_cli_round_trip(dev, scene_dir, tmp_path):
    from brush_amd import Splats

    out_ply, out_json = str(tmp_path / "out.ply"), str(tmp_path / "log.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "30", "--init-count", "800",
                        "--filter3d", "--filter3d-every", "10", "--export", out_ply, "--json", out_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_json) as f:
        log = json.load(f)
    assert log["filter3d"] is True and log["filter3d_refreshes"][:3] == [0, 10, 20] and len(log["losses"]) == 30
    back = Splats.from_ply(out_ply, dev)
    assert back.num_splats() == log["num_splats"] > 0
    import torch

    assert bool(torch.isfinite(back.log_scales).all()) and bool(torch.isfinite(back.raw_opacity).all())
    # python -m brush_amd.eval --zoom Z --image-dir DIR: the zoomed renders of the scored views, nothing else changes
    from PIL import Image

    from brush_amd.eval import main as eval_main, zoomed_camera
    from brush_amd.train_loop import load_dataset

    img_dir = str(tmp_path / "zoom")
    assert eval_main([out_ply, scene_dir, "--zoom", "4", "--image-dir", img_dir]) == 0
    views = load_dataset(scene_dir)[0].eval.views
    stems = [os.path.splitext(os.path.basename(v.name))[0] for v in views]
    assert sorted(os.listdir(img_dir)) == sorted(f"{st}_zoom4.png" for st in stems) and len(stems) == 2
    view = views[0]
    with torch.no_grad():
        want, _ = back.render(zoomed_camera(view.camera, (64, 64), 4.0), (64, 64))
    want = torch.clamp(torch.round(want[..., :3] * 255.0), 0, 255).to(torch.uint8).cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(os.path.join(img_dir, f"{stems[0]}_zoom4.png"))), want)


# ---------------------------------------------------------------------------- 5. what the feature is for
def _row_width(img, row):
    return int((img[row, :, 3] > 1.0 / 255.0).sum())


def test_zoom_in_keeps_a_subpixel_splat_a_blob(dev):
    """One splat, thin along the image's x axis (s = f / 16) and 3 f wide along the other two, in front of one
    "training" camera (fx = 64 px at 4 units: f = sqrt(0.2) 4 / 64), its centre on a pixel centre.  With
    sigma_x(Z) = sqrt(0.3 + (Z sigma3 fx / z)^2) pixels (0.3: the rasterizer's blur) and peak opacity P, the pixels of the
    centre row with alpha >= 1 / 255 are those within R = sigma_x sqrt(2 ln(255 P)) of the centre: 2 floor(R) + 1 of
    them, so  2 R - 1 <= width <= 2 R + 1.
      raw at 8x:    sigma3 = s, P <= 1:  width <= 2 sqrt(0.3 + (8 s fx / z)^2) sqrt(2 ln 255) + 1  (< 5: the blur floor)
      baked at Zx:  sigma3 = sqrt(s^2 + f^2), P = sigmoid(o) c: both inequalities, at Z = 1 and Z = 8
    (the bounds come from the formulas; they are asserted to sit 0.02 px away from a pixel boundary before the GPU is
    asked)."""
    import torch

    from brush_amd import Camera, Splats, filter3d_rates
    from brush_amd.camera import focal_to_fov

    w = h = 64
    fx, z, o = 64.0, 4.0, 6.0
    uv = (32.5 / 64.0, 32.5 / 64.0)
    cam = lambda zoom: Camera([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], focal_to_fov(fx * zoom, w),
                              focal_to_fov(fx * zoom, h), uv)
    means = torch.tensor([[0.0, 0.0, z]], device=dev)
    filt = filter3d_rates(means, [(cam(1), (w, h))])
    f = float(filt[0])
    assert abs(f - math.sqrt(0.2) * z / fx) <= 4 * U * f
    s, a = f / 16.0, 3.0 * f
    splats = Splats(means, torch.full((1, 1, 3), 2.0, device=dev), torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev),
                    torch.tensor([o], device=dev), torch.log(torch.tensor([[s, a, a]], device=dev)))
    baked = splats.bake_filter3d(filt)
    _, _, c, p = F.apply64(_np(splats.log_scales), [o], [f])
    k = math.sqrt(2.0 * math.log(255.0 * p[0]))
    sig3 = math.sqrt(s * s + f * f)
    R = {zoom: math.sqrt(0.3 + (zoom * sig3 * fx / z) ** 2) * k for zoom in (1, 8)}
    R_raw = math.sqrt(0.3 + (8.0 * s * fx / z) ** 2) * math.sqrt(2.0 * math.log(255.0))
    for r in R.values():
        assert 0.02 <= r - math.floor(r) <= 0.98
    widths, areas = {}, {}
    with torch.no_grad():
        for name, sp in (("raw", splats), ("baked", baked)):
            for zoom in (1, 8):
                img = _np(sp.render(cam(zoom), (w, h))[0])
                widths[name, zoom] = _row_width(img, 32)
                areas[name, zoom] = int((img[..., 3] > 1.0 / 255.0).sum())
    print(f"zoom: predicted R baked {R}, raw 8x <= {R_raw:.3f}; widths {widths}; areas {areas}; c = {c[0]:.4f}")
    MARGINS["zoom"] = {"widths": {f"{k[0]}_{k[1]}x": v for k, v in widths.items()},
                       "areas": {f"{k[0]}_{k[1]}x": v for k, v in areas.items()},
                       "predicted_half_width_baked": {str(k): v for k, v in R.items()}, "raw_8x_half_width_bound": R_raw}
    assert 1 <= widths["raw", 8] <= 2.0 * R_raw + 1.0 < 5.0
    for zoom in (1, 8):
        assert 2.0 * R[zoom] - 1.0 <= widths["baked", zoom] <= 2.0 * R[zoom] + 1.0, (zoom, widths)
    assert widths["baked", 8] >= 3 * widths["raw", 8] and widths["baked", 8] > 4 * widths["baked", 1]
    assert areas["baked", 8] > areas["raw", 8]
