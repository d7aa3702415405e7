"""The view-record kernels (brush_amd/csrc/view_records.hip) in one process, through the C ABI, on hand-built records of
1 to 17 views (tests/view_records_ref.py): no process group, no collectives.

Dense form (brush_reduce_view_records), every case in both buffer layouts and on three states of the index buffer
(all-ones, random words of which half point below the view's row count, left over from a reduction of other records):
  * v_means, v_scales, v_quats, v_opac equal the strictly sequential float32 sum in view order BIT FOR BIT (the planted
    payloads change their bits under any other order: tests/test_view_records_cpu.py), rows of unseen splats are +0,
    nothing outside the five arrays is written (NaN guards, inter-array padding, the v_xy segment);
  * v_sh is gated per element against float64: |gpu - f64| <= K(deg) eps32 sum_v |v_rgb_c(v)|, K = 4 x the error of a
    plain numpy float32 restatement on the same inputs.  Measured base values (CPU, degree 0..4): 0.515, 0.842, 1.834,
    4.095, 7.146, so K = 2.08, 3.4, 7.36, 16.4, 28.6 (VR.K_BASE, VR.k_sh);
  * the six results are bit-identical, and every index entry a reduction consumed reads 0xFFFFFFFF afterwards.
Adam form (brush_reduce_view_records_adam): the post-state against tests/ref64.adam64 fed the pre-state and the dense
form's sums (gated first), with the allowances of tests/test_gpu_optimizer_f64.py::_check_groups; the densification
statistics bit for bit; next_quats_fed within the 4 ulp of test_normalize_quats_within_few_ulp; both layouts the same bits.
Record writer (brush_render_backward_records), deterministic mode: the records against the dense backward of the same
render bit for bit, and truncation at max_rows.
Worst ratios go to tests/margins.py, section view_records."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from tests import helpers as H
from tests import margins
from tests import ref64 as R64
from tests import view_records_ref as VR
from tests.test_gpu_optimizer_f64 import B1, B2, EPS, LERP, LRS, _check_groups, _params, _signed_log

pytestmark = pytest.mark.gpu

GUARD = 16                 # NaN floats on either side of the gradient block
NAN_BITS = 0x7FC00000      # what torch.full(nan) writes
SUMS = ("v_means", "v_scales", "v_quats", "v_opac")


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=4)
def _refs(W, n, deg):
    """The two layouts of one case and its references, computed once and shared (read-only)."""
    seed = VR.case_seed(W, n, deg)
    cases = {lay: VR.directed_views(n, W, deg, seed, lay) for lay in ("padded", "packed")}
    other = {lay: VR.directed_views(n, W, deg, seed + 1, lay) for lay in ("padded", "packed")}
    f32, f64 = VR.reduce_f32(cases["padded"]), VR.reduce_f64(cases["padded"])
    for d in (f32, f64):
        for a in d.values():
            a.setflags(write=False)
    return cases, other, f32, f64


class _Views:
    """One case's buffers on the device."""

    def __init__(self, dev, case):
        import torch

        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.case = case
        self.records = t(case["records"])
        self.view_rows = t(case["view_rows"].view(np.int32))
        self.offsets = None if case["view_offsets"] is None else t(case["view_offsets"].view(np.int32))
        self.campos, self.means = t(case["campos"]), t(case["means"])
        assert self.records.data_ptr() % 16 == 0

    def head(self):
        c = self.case
        return (self.records.data_ptr(), c["W"], c["rows_per_view"], self.view_rows.data_ptr(),
                None if self.offsets is None else self.offsets.data_ptr(), self.campos.data_ptr())


def _index_tensor(dev, words):
    import torch

    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(dev)


def _index_words(t):
    return t.cpu().numpy().view(np.uint32)


def _random_index(rng, case):
    """Random u32 words; half of the entries of a view are below its row count, so that they pass the range check and
    the kernel has to compare the gid of the record they point to."""
    n, W = case["n"], case["W"]
    idx = rng.integers(0, 2 ** 32, (W, n), dtype=np.uint64).astype(np.uint32)
    low = rng.random((W, n)) < 0.5
    for v in range(W):
        rows = max(1, min(int(case["view_rows"][v]), case["rows_per_view"]))
        idx[v, low[v]] = rng.integers(0, rows, int(low[v].sum()))
    return idx.reshape(-1)


def _reduce_dense(dev, views, index):
    """brush_reduce_view_records into a NaN-filled block with NaN guards; returns the whole buffer."""
    import torch

    from brush_amd import _lib
    from brush_amd.render import grad_block_layout

    c = views.case
    n, W, deg = c["n"], c["W"], c["deg"]
    layout, total = grad_block_layout(n, (deg + 1) ** 2)
    buf = torch.full((GUARD + total + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    seg = lambda name: buf.data_ptr() + 4 * (GUARD + layout[name][0])
    assert index.numel() == n * W
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_reduce_view_records(
            *views.head(), views.means.data_ptr(), n, deg, seg("v_means"), seg("v_scales"), seg("v_quats"), seg("v_sh"),
            seg("v_opac"), index.data_ptr(), 4 * n * W, torch.cuda.current_stream().cuda_stream),
            "brush_reduce_view_records")
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _unpack(buf, n, ncoef):
    """The five arrays of the block; asserts that nothing else in the buffer was written."""
    from brush_amd.render import grad_block_layout

    layout, total = grad_block_layout(n, ncoef)
    b = buf.view(np.uint32)
    assert np.all(b[:GUARD] == NAN_BITS) and np.all(b[GUARD + total:] == NAN_BITS), "guard floats written"
    body = buf[GUARD:GUARD + total]
    used = np.zeros(total, bool)
    out = {}
    for name, shape in (("v_means", (n, 3)), ("v_scales", (n, 3)), ("v_quats", (n, 4)), ("v_opac", (n,)),
                        ("v_sh", (n, ncoef, 3))):
        off, sz = layout[name]
        used[off:off + sz] = True
        out[name] = body[off:off + sz].reshape(shape)
    assert np.all(body.view(np.uint32)[~used] == NAN_BITS), "inter-array padding or the v_xy segment written"
    return out


def _check_dense(out, f32, f64, deg):
    """The dense form's gate; returns the worst v_sh ratio in units of eps32 mag_sh."""
    unseen = f32["views_seen"] == 0
    for k in SUMS + ("v_sh",):
        assert not np.isnan(out[k]).any(), k
        assert not VR.bits(out[k])[unseen].any(), f"{k}: rows of unseen splats must be +0"
    for k in SUMS:
        bad = np.argwhere(VR.bits(out[k]) != VR.bits(f32[k]))
        assert len(bad) == 0, (k, len(bad), bad[0], out[k][tuple(bad[0])], f32[k][tuple(bad[0])])
    worst, nbad = VR.sh_gate(out["v_sh"], f64["v_sh"], f64["mag_sh"], deg)
    assert nbad == 0, (worst, VR.k_sh(deg), nbad)
    return worst


def _consumed_cleared(index, case):
    w = _index_words(index).reshape(case["W"], case["n"])
    return bool(np.all(w[case["vis"].T] == VR.INVALID))


@pytest.mark.parametrize("W,n,deg", VR.DENSE_CASES)
def test_dense_sum_is_the_sequential_float32_sum(dev, W, n, deg):
    cases, other, f32, f64 = _refs(W, n, deg)
    rng = np.random.default_rng(VR.case_seed(W, n, deg))
    results = {}
    worst = 0.0
    for lay in ("padded", "packed"):
        views, views_other = _Views(dev, cases[lay]), _Views(dev, other[lay])
        ones = _index_tensor(dev, np.full(n * W, VR.INVALID, np.uint32))
        results[lay, "ones"] = _reduce_dense(dev, views, ones)
        assert np.all(_index_words(ones) == VR.INVALID), "an all-ones index must stay all-ones"
        rnd = _index_tensor(dev, _random_index(rng, cases[lay]))
        results[lay, "random"] = _reduce_dense(dev, views, rnd)
        assert _consumed_cleared(rnd, cases[lay])
        left = _index_tensor(dev, _random_index(rng, other[lay]))
        _reduce_dense(dev, views_other, left)        # another record set of the same n leaves its traces ...
        assert _consumed_cleared(left, other[lay])
        results[lay, "leftover"] = _reduce_dense(dev, views, left)   # ... which must not matter
        assert _consumed_cleared(left, cases[lay])
    first = results["padded", "ones"]
    worst = _check_dense(_unpack(first, n, (deg + 1) ** 2), f32, f64, deg)
    for key, buf in results.items():
        assert np.array_equal(buf.view(np.uint32), first.view(np.uint32)), f"{key} differs from padded / all-ones"
    print(f"view records dense W={W} n={n} deg={deg}: v_sh worst {worst:.3f} eps32 mag (K {VR.k_sh(deg):.2f}); "
          f"seen {int((f32['views_seen'] > 0).sum())} of {n}, planted {len(cases['padded']['planted'])}")
    margins.record("view_records", "v_sh", worst / VR.k_sh(deg))
    margins.check_growth("view_records", "v_sh", worst / VR.k_sh(deg))


# ---- Adam form ------------------------------------------------------------------------------------------------------

def _adam_state(rng, case, ncoef):
    n = case["n"]
    x = _params(rng, n, ncoef)
    x[0] = case["means"].copy()     # the reduction takes the SH directions from the means it steps
    total = n * (11 + 3 * ncoef)
    acc = (rng.random(n) * 10.0).astype(np.float32)
    cnt = rng.integers(0, 50, n).astype(np.float32)
    cnt[rng.random(n) < 0.1] = -0.0
    return dict(x=[np.ascontiguousarray(a.reshape(-1)) for a in x], m1=_signed_log(rng, (total,), -12, 2),
                m2=(10.0 ** rng.uniform(-12, 6, size=total)).astype(np.float32), acc=acc, cnt=cnt)


def _reduce_adam(dev, views, pre, time, vjp):
    import torch

    from brush_amd import _lib

    c = views.case
    n, W, deg = c["n"], c["W"], c["deg"]
    t = lambda a: torch.from_numpy(a.copy()).to(dev)
    x = [t(a) for a in pre["x"]]
    m1, m2, acc, cnt = t(pre["m1"]), t(pre["m2"]), t(pre["acc"]), t(pre["cnt"])
    nq = torch.full((n, 4), float("nan"), dtype=torch.float32, device=dev)
    index = _index_tensor(dev, np.full(n * W, VR.INVALID, np.uint32))
    cfg = _lib.BrushAdamConfig(LRS[0], LRS[1], LRS[2], LRS[3], LRS[4], float(LERP), B1, B2, EPS, time, vjp, float(W))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().brush_reduce_view_records_adam(
            *views.head(), C.byref(cfg), 64, 48, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr(),
            x[4].data_ptr(), n, deg, m1.data_ptr(), m2.data_ptr(), nq.data_ptr(), acc.data_ptr(), cnt.data_ptr(),
            index.data_ptr(), 4 * n * W, torch.cuda.current_stream().cuda_stream), "brush_reduce_view_records_adam")
    torch.cuda.synchronize()
    assert np.all(_index_words(index) == VR.INVALID)
    g = lambda a: a.cpu().numpy()
    return dict(x=[g(a) for a in x], m1=g(m1), m2=g(m2), acc=g(acc), cnt=g(cnt), nq=g(nq))


ADAM_CASES = [(n, deg, W, vjp, time) for n in (257, 4096, 4099) for deg in (0, 3, 4) for W in (8, 9) for vjp in (0, 1)
              for time in (1, 1000)]


@pytest.mark.parametrize("n,deg,W,vjp,time", ADAM_CASES)
def test_adam_form_steps_with_the_sequential_sums(dev, n, deg, W, vjp, time):
    cases, _, f32, f64 = _refs(W, n, deg)
    ncoef = (deg + 1) ** 2
    padded, packed = _Views(dev, cases["padded"]), _Views(dev, cases["packed"])
    ones = _index_tensor(dev, np.full(n * W, VR.INVALID, np.uint32))
    dense = _unpack(_reduce_dense(dev, padded, ones), n, ncoef)
    worst_sh = _check_dense(dense, f32, f64, deg)      # the gradients the reference is fed are gated first
    pre = _adam_state(np.random.default_rng([n, deg, W, vjp, time]), cases["padded"], ncoef)
    seen = f32["views_seen"] > 0
    pre["cnt"][np.flatnonzero(~seen)[:2]] = -0.0       # "untouched" is visible on these: -0 + 0 would be +0
    post = _reduce_adam(dev, padded, pre, time, vjp)
    pre["g"] = [dense[k].reshape(-1) for k in SUMS + ("v_sh",)]      # unseen splats: gradient +0
    st = types.SimpleNamespace(n=n, ncoef=ncoef, sizes=[3 * n, 3 * n, 4 * n, n, 3 * ncoef * n])
    res, (nsub, nchain) = _check_groups(st, pre, post, time, vjp)
    worst = max(max(r["x"], r["m"], r["v"]) for r in res.values())
    # densification statistics (train.rs:284-316): plain float32 operations, bit for bit
    want_acc = pre["acc"] + f32["xy_norm"] * np.float32(W)
    assert want_acc.dtype == np.float32 and np.array_equal(VR.bits(post["acc"]), VR.bits(want_acc))
    want_cnt = np.where(seen, pre["cnt"] + f32["views_seen"], pre["cnt"]).astype(np.float32)
    assert np.array_equal(VR.bits(post["cnt"]), VR.bits(want_cnt))
    assert np.signbit(post["cnt"][~seen]).any(), "no untouched -0 count to look at"
    # what the next forward is fed: the stepped rotation, normalised (|q|^2, sqrtf and an IEEE division: 4 ulp)
    q = post["x"][2].reshape(n, 4).astype(np.float64)
    want_q = q / np.linalg.norm(q, axis=1, keepdims=True)
    wq, iq, bad_q = R64.gate(post["nq"], want_q, 4.0 * R64.spacing32(want_q))
    assert bad_q == 0, (wq, iq)
    again = _reduce_adam(dev, packed, pre, time, vjp)
    for k in ("m1", "m2", "acc", "cnt", "nq"):
        assert np.array_equal(VR.bits(again[k]), VR.bits(post[k])), f"packed layout: {k} differs"
    for i in range(5):
        assert np.array_equal(VR.bits(again["x"][i]), VR.bits(post["x"][i])), f"packed layout: x{i} differs"
    print(f"view records adam n={n} deg={deg} W={W} vjp={vjp} time={time}: worst err/tol {worst:.3f}, next_quats "
          f"{wq:.3f} of 4 ulp, v_sh {worst_sh:.3f} eps32 mag; subnormal-priced {nsub}, chain-priced {nchain}")
    margins.record("view_records", "adam", worst)
    margins.check_growth("view_records", "adam", worst)


# ---- record writer --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,w,h,deg", [(3000, 160, 96, 2), (65, 64, 48, 0)])
def test_record_writer_matches_the_dense_backward_bit_for_bit(dev, n, w, h, deg):
    """Deterministic mode: the records backward and the dense backward of one render read the same compact sums and run
    the same splat_projection_vjp, so record words 1..11 are the dense rows of the splat, Y0 v_rgb is its v_sh dc row,
    word 15 is sqrt((v_xy.x w/2)^2 + (v_xy.y h/2)^2) in float32, word 0 the gid, rows in compact (depth) order;
    exactly min(V, max_rows) rows are written."""
    import torch

    import brush_amd
    from brush_amd import _lib
    from brush_amd import render as R

    ncoef = (deg + 1) ** 2
    cloud = H.synthetic_cloud(n, deg, seed=21, mean_mult=0.002)
    p = {k: torch.from_numpy(v).to(dev) for k, v in cloud.items()}
    c = H.reference_test_camera(w, h)
    cam = brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])
    out, aux, u = R._forward_impl(cam, (w, h), p["means"], p["log_scales"], p["quats"], p["sh"], p["raw_opac"], False,
                                  None, deterministic=True)
    V = aux.read_num_visible()
    assert 8 <= V < n
    v_out = (torch.randn((h, w, 4), generator=torch.Generator().manual_seed(3)) / (h * w)).to(dev)
    g, _ = R._backward_impl(u, aux, p["means"], p["log_scales"], p["quats"], p["raw_opac"], ncoef, out, v_out)
    dense = {k: t.cpu().numpy() for k, t in g.items()}
    gids = aux.global_from_compact_gid[:V].cpu().numpy().astype(np.int64)
    l = _lib.lib()
    nbytes = C.c_size_t()
    _lib.check(l.brush_bwd_workspace_size_flags(n, w, h, deg, int(aux.max_intersects), aux.workspace_flags,
                                                C.byref(nbytes)), "brush_bwd_workspace_size_flags")
    cap = V + 8

    def records(max_rows, null=False):
        buf = torch.full((cap, VR.REC), float("nan"), dtype=torch.float32, device=dev)
        ws, s = aux.backward_workspace(nbytes.value, dev)
        with torch.cuda.device(dev):
            _lib.check(l.brush_render_backward_records(
                C.byref(u), C.byref(s), p["means"].data_ptr(), p["log_scales"].data_ptr(), p["quats"].data_ptr(),
                p["raw_opac"].data_ptr(), n, out.data_ptr(), v_out.data_ptr(), None if null else buf.data_ptr(),
                max_rows, ws.data_ptr(), nbytes.value, torch.cuda.current_stream().cuda_stream),
                "brush_render_backward_records")
        torch.cuda.synchronize()
        return buf.cpu().numpy()

    full = records(V + 7)
    assert np.all(full.view(np.uint32)[V:] == NAN_BITS), "rows behind the visible ones written"
    rec = full[:V]
    assert np.array_equal(rec[:, 0].view(np.uint32), gids.astype(np.uint32)), "word 0 / compact order"
    mismatches = {}
    for name, lo, hi in (("v_means", 1, 4), ("v_scales", 4, 7), ("v_quats", 7, 11), ("v_opac", 11, 12)):
        want = dense[name][gids].reshape(V, hi - lo)
        mismatches[name] = int((VR.bits(rec[:, lo:hi]) != VR.bits(want)).sum())
    y0 = np.float32(0.2820947917738781)
    mismatches["Y0 v_rgb"] = int((VR.bits(y0 * rec[:, 12:15]) != VR.bits(dense["v_sh"][gids, 0, :])).sum())
    vx = dense["v_xy"][gids, 0] * np.float32(w / 2.0)
    vy = dense["v_xy"][gids, 1] * np.float32(h / 2.0)
    norm = np.sqrt(vx * vx + vy * vy)
    assert norm.dtype == np.float32
    mismatches["norm"] = int((VR.bits(rec[:, 15]) != VR.bits(norm)).sum())
    print(f"record writer n={n} {w}x{h} deg={deg}: V={V}, words differing from the dense backward {mismatches}")
    assert not any(mismatches.values()), mismatches
    assert np.abs(rec[:, 1:]).max() > 0
    for max_rows in (V, V - 1, 1, 0):
        got = records(max_rows, null=max_rows == 0)
        k = min(V, max_rows)
        assert np.array_equal(got.view(np.uint32)[:k], full.view(np.uint32)[:k]), max_rows
        assert np.all(got.view(np.uint32)[k:] == NAN_BITS), f"max_rows={max_rows}: more than {k} rows written"
