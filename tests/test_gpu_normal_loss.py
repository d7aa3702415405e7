"""Normal maps and the depth-normal consistency loss on the GPU: brush_splat_normals, its VJP and brush_normal_loss
against the numpy float32 restatement of tests/normal_ref64.py bit for bit (and, for the VJP, float64 autograd within the
running bound derived there), NULL outputs, the normals-only form, repeatability and graph replay; render_normals and
its autograd against the manual composition of the bare calls; the trainer option (off: the trainer without it; on: the
manual composition, alone and with depth supervision); a small scene trained with and without the term.

What goes through the feature replay's float transpose (the gradient of the rendered normal map at the per-splat
normals) is order dependent in its last bits.  Its allowance is the one tests/test_gpu_features.py derives for two runs
of that transpose, 2 (6 + P) U sum|fac v| with P <= 4 quadrants x tiles partial sums per row, pushed through the
splat-normal VJP, which is linear in v_normals: the VJP is run on the three unit vectors, and the allowance of word i of
a row is sum_c |VJP(e_c)_i| tol_c."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import features_ref64 as FR
from tests import normal_ref64 as NR
from tests import test_gpu_depth_loss as TD
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

F = np.float32
U = NR.U


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = _np(t) if not isinstance(t, np.ndarray) else t
    return np.ascontiguousarray(a).view(np.uint32)


def _tt(a, dev):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ratio(got, want, tol):
    return FR.ratio(_np(got) if not isinstance(got, np.ndarray) else got, want, tol)


# ---------------------------------------------------------------------------- 1. splat normals
def _view_uniforms(viewmat):
    from brush_amd import _lib as L

    u = L.BrushUniforms()
    u.viewmat[:] = [float(x) for x in viewmat]
    u.img_size[:] = [1, 1]
    return u


@pytest.mark.parametrize("n", [1, 63, 65, 1000])
@pytest.mark.parametrize("seed", [0, -1])
def test_splat_normals_and_their_vjp_match_the_restatement_bitwise(dev, n, seed):
    import torch

    from brush_amd.normal_loss import splat_normals_backward_into, splat_normals_from

    s = NR.make_splats(n, seed)
    want, k, sign = NR.splat_normals32(s["viewmat"], s["means"], s["log_scales"], s["quats"])
    u = _view_uniforms(s["viewmat"])
    means, log_scales, quats = (_tt(s[key], dev) for key in ("means", "log_scales", "quats"))
    out = torch.full((n, 3), float("nan"), device=dev)
    got = splat_normals_from(u, means, log_scales, quats, out=out)
    assert np.array_equal(_bits(got), _bits(want))  # every row written: behind the camera, ties, dot == 0
    if n >= 8:
        vm = s["viewmat"].astype(np.float64).reshape(4, 4)
        z = (s["means"].astype(np.float64) @ vm[:3, :3] + vm[3, :3])[:, 2]
        assert (z < 0).any() and (z > 0).any() and (sign == -1).any() and (sign == 1).any()
        assert list(k[1:5]) == [1, 0, 0, 2]
        if seed == -1:
            assert sign[5] == 1 and np.array_equal(_np(got)[5], np.array([0, 0, 1], F))  # dot == 0 exactly
    # the VJP accumulates into a non-zero v_quats
    v_normals = _tt(s["v_normals"], dev)
    v_quats = _tt(s["v_quats0"], dev).clone()
    splat_normals_backward_into(u, means, log_scales, quats, v_normals, v_quats)
    want_q = NR.splat_normals_backward32(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"],
                                         s["v_quats0"])
    assert np.array_equal(_bits(v_quats), _bits(want_q))
    # ... and, from zero, is float64 autograd of the rotation matrix's column within the running bound
    zero = torch.zeros((n, 4), device=dev)
    splat_normals_backward_into(u, means, log_scales, quats, v_normals, zero)
    _, g64 = NR.splat_normals64(s["viewmat"], s["quats"], k, sign, s["v_normals"])
    _, e, _, _ = NR.splat_vjp_bound(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"])
    r = _ratio(zero, g64, e)
    print(f"splat normal VJP n={n} seed={seed}: |gpu - f64| / bound {r:.4f}")
    assert 0.0 < r <= 1.0


def test_splat_normals_autograd_reaches_the_quaternions_only(dev):
    import torch

    import brush_amd

    s = NR.make_splats(65, 0)
    means, log_scales, quats = (_tt(s[key], dev).requires_grad_(True) for key in ("means", "log_scales", "quats"))
    u = _view_uniforms(s["viewmat"])
    normals = brush_amd.splat_normals(u, means, log_scales, quats)
    v = _tt(s["v_normals"], dev)
    (normals * v).sum().backward()
    assert means.grad is None and log_scales.grad is None
    want = NR.splat_normals_backward32(s["viewmat"], s["means"], s["log_scales"], s["quats"], s["v_normals"],
                                       np.zeros((65, 4), F))
    assert np.array_equal(_bits(quats.grad), _bits(want))
    assert tuple(brush_amd.splat_normals(u, means[:0], log_scales[:0], quats[:0]).shape) == (0, 3)


# ---------------------------------------------------------------------------- 2. the pixel kernel
# (513, 512): 33 x 32 = 1056 tiles, more than the grid cap of 1024 workgroups: the first 32 stride to a second tile.
SHAPES = [(1, 1), (2, 5), (3, 3), (5, 5), (33, 31), (130, 67), (513, 512)]
_CASES = {}


def _case(w, h):
    """Inputs and the float32 restatement of one shape, computed once, shared and left unchanged."""
    if (w, h) not in _CASES:
        c = NR.make_case(w, h, bad=w * h >= 1000)
        ref = NR.normal_loss32(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], c["alpha_min"],
                               c["v_pred"][..., 3])
        pred = np.random.default_rng(w + 7 * h).random((h, w, 4), dtype=F)
        pred[..., 3] = c["alpha"]
        _CASES[(w, h)] = (c, pred, ref)
    return _CASES[(w, h)]


def _pixel_uniforms(c):
    from brush_amd import _lib as L

    u = L.BrushUniforms()
    u.img_size[:] = [c["w"], c["h"]]
    u.tile_bounds[:] = [-(-c["w"] // 16), -(-c["h"] // 16)]
    u.focal[:] = [float(c["intr"][0]), float(c["intr"][1])]
    u.pixel_center[:] = [float(c["intr"][2]), float(c["intr"][3])]
    return u


def _abi(dev, c, pred, depth, normals_img, dn=None, v_depth=None, v_normals=None, v_pred=None, stats=None, accum=None,
         ws=None):
    """brush_normal_loss on preallocated torch tensors (None: NULL)."""
    import torch

    from brush_amd import _lib as L
    from brush_amd.normal_loss import workspace_bytes

    cfg = L.BrushNormalLoss(c["weight"], c["alpha_min"])
    n = workspace_bytes(c["w"], c["h"])
    ws = torch.empty(n, dtype=torch.uint8, device=dev) if ws is None else ws
    stats = torch.empty(2, dtype=torch.float32, device=dev) if stats is None else stats
    p = lambda t: None if t is None else t.data_ptr()
    u = _pixel_uniforms(c)
    L.check(L.lib().brush_normal_loss(C.byref(u), pred.data_ptr(), depth.data_ptr(), p(normals_img), C.byref(cfg),
                                      p(dn), p(v_depth), p(v_normals), p(v_pred), stats.data_ptr(), p(accum),
                                      ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream), "brush_normal_loss")
    return stats


SENTINEL = 7.0


def _outputs(dev, w, h, v_pred0):
    import torch

    return dict(dn=torch.full((h, w, 3), SENTINEL, device=dev), v_depth=torch.full((h, w), SENTINEL, device=dev),
                v_normals=torch.full((h, w, 3), SENTINEL, device=dev), v_pred=v_pred0.clone())


@pytest.mark.parametrize("w,h", SHAPES)
def test_pixel_kernel_matches_the_restatement_bitwise(dev, w, h):
    import torch

    from brush_amd.normal_loss import workspace_bytes

    c, pred_np, ref = _case(w, h)
    valid, share = ref["valid"], float(ref["valid"].mean())
    if w * h >= 1000:  # (the masks themselves are checked on the CPU, tests/test_normal_cpu.py)
        assert 0.25 <= share <= 0.75, share
        for rule in ("low_alpha", "zero_depth", "nonfinite", "overflow"):
            assert ref[rule].any(), rule
        assert np.isnan(c["alpha"]).any() and np.isnan(c["depth"]).any() and np.isinf(c["depth"]).any()
    else:
        assert int(valid.sum()) == max(w - 2, 0) * max(h - 2, 0)
    pred, depth, nimg, v_pred0 = (_tt(a, dev) for a in (pred_np, c["depth"], c["normals_img"], c["v_pred"]))
    o = _outputs(dev, w, h, v_pred0)
    accum = torch.tensor([0.37], device=dev)
    stats = _np(_abi(dev, c, pred, depth, nimg, accum=accum, **o))
    assert np.array_equal(_bits(o["dn"]), _bits(ref["depth_normals"]))
    assert np.array_equal(_bits(o["v_depth"]), _bits(ref["v_depth"]))
    assert np.array_equal(_bits(o["v_normals"]), _bits(ref["v_normals_img"]))
    got = _np(o["v_pred"])
    assert np.array_equal(_bits(got[..., 3]), _bits(ref["v_pred_alpha"]))
    assert np.array_equal(_bits(got[..., :3]), _bits(c["v_pred"][..., :3]))  # the colour channels are never touched
    assert np.array_equal(_bits(got[~ref["touched"]]), _bits(c["v_pred"][~ref["touched"]]))
    print(f"normal loss {w}x{h}: valid {share:.4f}, stats {stats!r} vs {ref['stats']!r}")
    assert np.array_equal(_bits(stats), _bits(ref["stats"]))
    assert _np(accum)[0] == F(0.37) + stats[0]  # loss_accum: one f32 add
    if not valid.any():  # (1,1), (2,5): nothing valid, loss 0, all-zero gradients, v_pred untouched
        assert stats[0] == 0 and stats[1] == 0 and np.array_equal(_bits(got), _bits(c["v_pred"]))
        assert not _bits(o["v_depth"]).any() and not _bits(o["v_normals"]).any() and not _bits(o["dn"]).any()
    else:
        assert stats[0] > 0 and (got[..., 3][valid] != c["v_pred"][..., 3][valid]).any()
        assert _np(o["v_depth"]).any()
    if (w, h) == (5, 5):  # the centre pixel gathers from four valid centres
        assert valid[1:4, 1:4].all() and _np(o["v_depth"])[2, 2] != 0
    assert workspace_bytes(w, h) <= 16384


@pytest.mark.parametrize("w,h", [(33, 31), (130, 67), (513, 512)])
def test_repeatable_null_outputs_normals_only_and_graph_replay(dev, w, h):
    import torch

    from brush_amd import _lib as L
    from brush_amd.normal_loss import workspace_bytes

    c, pred_np, ref = _case(w, h)
    pred, depth, nimg, v_pred0 = (_tt(a, dev) for a in (pred_np, c["depth"], c["normals_img"], c["v_pred"]))
    keys = ("dn", "v_depth", "v_normals", "v_pred")

    def run(skip=()):
        o = _outputs(dev, w, h, v_pred0)
        for k in skip:
            o[k] = None
        return o, _abi(dev, c, pred, depth, nimg, **o)

    (first, stats), (again, stats2) = run(), run()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(stats), _bits(stats2)) and np.array_equal(_bits(stats), _bits(ref["stats"]))
    for k in keys:
        assert np.array_equal(_bits(first[k]), _bits(again[k])), k
    # NULL outputs: every remaining output and the statistics keep their bits
    for skip in (("dn",), ("v_depth",), ("v_normals",), ("v_pred",), ("dn", "v_pred"), keys):
        o, st = run(skip)
        assert np.array_equal(_bits(st), _bits(stats)), skip
        for k in keys:
            if k not in skip:
                assert np.array_equal(_bits(o[k]), _bits(first[k])), (skip, k)
    # the normals-only form: the depth-derived normals and the valid fraction alone
    dn = torch.full((h, w, 3), SENTINEL, device=dev)
    st = _np(_abi(dev, c, pred, depth, None, dn=dn))
    assert np.array_equal(_bits(dn), _bits(first["dn"])) and st[0] == 0 and st[1] == ref["stats"][1]
    only = NR.normal_loss32(c["intr"], c["alpha"], c["depth"], None, c["weight"], c["alpha_min"])
    assert np.array_equal(_bits(st), _bits(only["stats"]))
    # ... which has no gradients to write: a gradient pointer without normals_img is refused, as aliasing is
    cfg, u = L.BrushNormalLoss(1.0, 0.5), _pixel_uniforms(c)
    ws = torch.empty(workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    call = lambda normals, v_depth, v_pred, ws_bytes=ws.numel(): L.lib().brush_normal_loss(
        C.byref(u), pred.data_ptr(), depth.data_ptr(), normals, C.byref(cfg), None, v_depth, None, v_pred,
        stats.data_ptr(), None, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert call(None, first["v_depth"].data_ptr(), None) != 0
    assert call(nimg.data_ptr(), depth.data_ptr(), None) != 0       # v_depth aliases depth
    assert call(nimg.data_ptr(), None, pred.data_ptr()) != 0        # v_pred aliases pred
    assert call(nimg.data_ptr(), None, None, 8) != 0                # workspace too small
    cfg.alpha_min = 0.0
    assert call(nimg.data_ptr(), None, None) != 0
    # graph capture and replay
    o = _outputs(dev, w, h, v_pred0)
    gstats = torch.zeros(2, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as torch's capture recipe asks
        _abi(dev, c, pred, depth, nimg, stats=gstats, ws=ws, **o)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _abi(dev, c, pred, depth, nimg, stats=gstats, ws=ws, **o)
    for _ in range(2):
        for k in ("dn", "v_depth", "v_normals"):
            o[k].fill_(SENTINEL)
        o["v_pred"].copy_(v_pred0), gstats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(gstats), _bits(stats))
        for k in keys:
            assert np.array_equal(_bits(o[k]), _bits(first[k])), k


def test_python_forms_are_the_kernel(dev):
    import torch

    import brush_amd

    w, h = 33, 31
    c, pred_np, ref = _case(w, h)
    pred, depth, nimg, v_pred0 = (_tt(a, dev) for a in (pred_np, c["depth"], c["normals_img"], c["v_pred"]))
    u = _pixel_uniforms(c)
    normals, frac = brush_amd.depth_normals(u, None, pred, depth, alpha_min=c["alpha_min"])
    assert np.array_equal(_bits(normals), _bits(ref["depth_normals"])) and _np(frac) == ref["stats"][1]
    v_pred = v_pred0.clone()
    other = torch.full((h, w), 0.25, device=dev)
    v_depth, v_normals, stats = brush_amd.normal_loss_into(u, pred, depth, nimg, v_pred, weight=c["weight"],
                                                           alpha_min=c["alpha_min"], v_depth_accum=other)
    assert v_depth is other and np.array_equal(_bits(v_depth), _bits((F(0.25) + ref["v_depth"]).astype(F)))
    assert np.array_equal(_bits(v_normals), _bits(ref["v_normals_img"]))
    assert np.array_equal(_bits(v_pred[..., 3]), _bits(ref["v_pred_alpha"]))
    assert np.array_equal(_bits(stats), _bits(ref["stats"]))
    # the differentiable form: the same loss, the three gradients scaled by the incoming scalar
    a, d, nn = pred.clone().requires_grad_(True), depth.clone().requires_grad_(True), nimg.clone().requires_grad_(True)
    loss = brush_amd.normal_consistency_loss(u, None, a, d, nn, weight=c["weight"], alpha_min=c["alpha_min"])
    assert loss.dim() == 0 and np.array_equal(_bits(loss).reshape(-1), _bits(ref["stats"][:1]))
    ga, gd, gn = torch.autograd.grad(loss * 2.0, [a, d, nn])
    zero_alpha = NR.normal_loss32(c["intr"], c["alpha"], c["depth"], c["normals_img"], c["weight"], c["alpha_min"])
    assert np.array_equal(_bits(ga[..., 3]), _bits((zero_alpha["v_pred_alpha"] * F(2.0)).astype(F)))
    assert not _bits(ga[..., :3]).any()
    assert np.array_equal(_bits(gd), _bits((ref["v_depth"] * F(2.0)).astype(F)))
    assert np.array_equal(_bits(gn), _bits((ref["v_normals_img"] * F(2.0)).astype(F)))
    with pytest.raises(ValueError, match="v_depth_accum"):
        brush_amd.normal_loss_into(u, pred, depth, nimg, None, v_depth_accum=torch.zeros((h, w + 1), device=dev))
    with pytest.raises(ValueError, match="alpha_min"):
        brush_amd.normal_loss_into(u, pred, depth, nimg, None, alpha_min=0.0)


# ---------------------------------------------------------------------------- 3. render_normals
W3 = H3 = 64
N3 = 192


def _camera(w, h, position=(0.0, 0.0, -8.0)):
    import brush_amd

    return brush_amd.Camera(list(position), [0.0, 0.0, 0.0, 1.0], 0.6, 0.6 * h / w, (0.5, 0.5))


def _small_scene(dev):
    """Seeded, of the kind tests/test_gpu_features.py renders: 180 opaque splats in a slab in front of the camera and 12
    far outside every frame, flattened along one axis each so that a shortest axis exists."""
    rng = np.random.default_rng(61)
    n = N3
    means = np.zeros((n, 3), F)
    means[:180, 0] = rng.uniform(-1.9, 1.9, 180)
    means[:180, 1] = rng.uniform(-1.9, 1.9, 180)
    means[:180, 2] = rng.uniform(-0.5, 0.5, 180)
    means[180:] = np.c_[rng.uniform(40.0, 60.0, 12), rng.uniform(40.0, 60.0, 12), np.zeros(12)]
    log_scales = (np.log(0.3) + rng.uniform(-0.15, 0.15, (n, 3))).astype(F)
    log_scales[np.arange(n), rng.integers(0, 3, n)] -= 1.2
    raw_opac = rng.uniform(2.0, 4.0, n).astype(F)
    quats = rng.normal(size=(n, 4))
    quats = (quats / np.linalg.norm(quats, axis=1, keepdims=True)).astype(F)
    quats = (quats / np.sqrt((quats.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(F)
    sh = rng.uniform(-0.5, 1.5, (n, 4, 3)).astype(F)
    return {k: _tt(v, dev) for k, v in dict(means=means, log_scales=log_scales, quats=quats, sh=sh,
                                            raw_opac=raw_opac).items()}


def _transpose_allowance(u, aux, v_img, n, w, h, dev):
    """[N,3] float64: what two runs of the float transpose of v_img may differ by (the module docstring)."""
    import torch

    from brush_amd.features import feature_grads_from_aux

    absg = torch.zeros((n, 3), device=dev)
    feature_grads_from_aux(u, aux, v_img.abs().contiguous(), absg)
    depth = FR.K_TREE + 4 * ((w + 15) // 16) * ((h + 15) // 16)
    return 2.0 * depth * U * _np(absg).astype(np.float64) * (1.0 + 2.0 * depth * U)


def _through_vjp(u, means, log_scales, quats, tol, dev):
    """[N,4] float64: sum_c |VJP(e_c)| tol[:, c], plus one rounding of the largest word for the kernel's own sums."""
    import torch

    from brush_amd.normal_loss import splat_normals_backward_into

    n = int(means.shape[0])
    out = np.zeros((n, 4))
    for ch in range(3):
        e = torch.zeros((n, 3), device=dev)
        e[:, ch] = 1.0
        g = torch.zeros((n, 4), device=dev)
        splat_normals_backward_into(u, means, log_scales, quats, e, g)
        out += np.abs(_np(g).astype(np.float64)) * (1.0 + 16 * U) * tol[:, ch:ch + 1]
    return out


def test_render_normals_is_the_composition_of_the_bare_calls(dev, deterministic):
    import torch

    import brush_amd
    from brush_amd import render as R
    from brush_amd.features import feature_grads_from_aux, features_from_aux
    from brush_amd.normal_loss import normal_loss_into, splat_normals_backward_into, splat_normals_from

    w, h, n = W3, H3, N3
    cam = _camera(w, h)
    t = _small_scene(dev)
    names = ("means", "log_scales", "quats", "sh", "raw_opac")
    for v in t.values():
        v.requires_grad_(True)
    img, depth, normals_img, aux = brush_amd.render_normals(cam, (w, h), t["means"], t["log_scales"], t["quats"],
                                                            t["sh"], t["raw_opac"])
    assert normals_img.shape == (h, w, 3) and normals_img.requires_grad and img.requires_grad and depth.requires_grad
    d = {k: v.detach() for k, v in t.items()}
    img2, depth2, aux2 = brush_amd.render_splats_depth(cam, (w, h), d["means"], None, d["log_scales"], d["quats"],
                                                       d["sh"], d["raw_opac"])
    assert np.array_equal(_bits(img), _bits(img2)) and np.array_equal(_bits(depth), _bits(depth2))
    u = R.pack_uniforms(cam, (w, h), 1, n)
    normals = splat_normals_from(u, d["means"], d["log_scales"], d["quats"])
    assert np.array_equal(_bits(normals_img), _bits(features_from_aux(u, aux2, normals)))
    assert np.array_equal(_bits(normals_img), _bits(features_from_aux(u, aux, normals)))
    assert float(img.detach()[..., 3].max()) > 0.9
    # the untracked form: the same bits, no graph
    with torch.no_grad():
        i3, d3, n3, _ = brush_amd.render_normals(cam, (w, h), d["means"], d["log_scales"], d["quats"], d["sh"],
                                                 d["raw_opac"])
    assert not n3.requires_grad and np.array_equal(_bits(n3), _bits(normals_img)) and np.array_equal(_bits(i3), _bits(img))
    assert np.array_equal(_bits(d3), _bits(depth))
    # the rendered normals agree with the splats': camera-facing, no longer than alpha
    nz = _np(normals_img)
    assert nz[..., 2].min() < -0.3 and np.linalg.norm(nz, axis=2).max() <= float(img.detach()[..., 3].max()) * (1 + 1e-5)
    # autograd of the loss against the manual composition
    kw = dict(weight=0.8, alpha_min=0.3)
    loss = brush_amd.normal_consistency_loss(cam, (w, h), img, depth, normals_img, **kw)
    grads = torch.autograd.grad(loss, [t[k] for k in names])
    bufs = R._depth_buffers(n, (w, h), dev)
    pred, aux_m, u_m = R._forward_impl(cam, (w, h), d["means"], d["log_scales"], d["quats"], d["sh"], d["raw_opac"],
                                       False, None, depth=bufs)
    nimg_m = features_from_aux(u_m, aux_m, splat_normals_from(u_m, d["means"], d["log_scales"], d["quats"]))
    v_pred = torch.zeros_like(pred)
    v_depth, v_nimg, stats = normal_loss_into(u_m, pred, bufs[0], nimg_m, v_pred, **kw)
    assert np.array_equal(_bits(loss).reshape(-1), _bits(stats[:1])) and 0.2 < float(stats[1]) < 0.98
    assert float(stats[0]) > 0
    g, _ = R._backward_impl(u_m, aux_m, d["means"], d["log_scales"], d["quats"], d["raw_opac"], 4, pred, v_pred,
                            depth=(bufs[1], v_depth))
    v_normals = torch.zeros((n, 3), device=dev)
    feature_grads_from_aux(u_m, aux_m, v_nimg, v_normals)
    render_quats = g["v_quats"].clone()
    splat_normals_backward_into(u_m, d["means"], d["log_scales"], d["quats"], v_normals, g["v_quats"])
    for k, got in zip(("v_means", "v_scales", "v_quats", "v_sh", "v_opac"), grads):
        assert bool(torch.isfinite(got).all()), k
        if k != "v_quats":
            assert np.array_equal(_bits(got), _bits(g[k])), k  # deterministic mode: to the bits
    tol_n = _transpose_allowance(u_m, aux_m, v_nimg, n, w, h, dev)
    tol_q = _through_vjp(u_m, d["means"], d["log_scales"], d["quats"], tol_n, dev)
    # (the sum with the render's own v_quats rounds once on either side)
    tol_q = tol_q + 2.0 * U * (np.abs(_np(g["v_quats"])) + tol_q)
    r = _ratio(grads[2], _np(g["v_quats"]).astype(np.float64), tol_q)
    print(f"render_normals v_quats: |autograd - manual| / allowance {r:.4f}")
    assert r <= 1.0
    assert not torch.equal(g["v_quats"], render_quats)  # the normals' own gradient is in there
    assert not bool(g["v_quats"][180:].any())           # the splats outside the frame receive nothing
    # Splats.render_normals is the same call on the normalised rotations
    s = brush_amd.Splats(d["means"], d["sh"], d["quats"] * 1.7, d["raw_opac"], d["log_scales"])
    with torch.no_grad():
        i4, d4, n4, _ = s.render_normals(cam, (w, h))
        rot = s.rotation.detach()
        nrm = (rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))).contiguous()
        i5, d5, n5, _ = brush_amd.render_normals(cam, (w, h), d["means"], d["log_scales"], nrm, d["sh"], d["raw_opac"])
    assert np.array_equal(_bits(n4), _bits(n5)) and np.array_equal(_bits(i4), _bits(i5))


# ---------------------------------------------------------------------------- 4. trainer
W, Hh, ALPHA_MIN, PATHS = TD.W, TD.Hh, TD.ALPHA_MIN, TD.PATHS


def test_trainer_with_the_term_off_is_the_trainer_without_the_option(dev, deterministic):
    import torch

    setup = TD._trainer_setup(dev)
    order = [0, 1, 1]
    for fused, deferred in PATHS:
        off = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order)
        zero = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order, normal_weight=0.0,
                               normal_from_step=0, normal_alpha_min=ALPHA_MIN)
        early = TD._run_trainer(dev, setup, fused, deferred, with_depth=False, order=order, normal_weight=0.4,
                                normal_from_step=3, normal_alpha_min=ALPHA_MIN)
        for on in (zero, early):
            assert on[0] == off[0], (fused, deferred)
            for k in off[1]:
                assert torch.equal(on[1][k], off[1][k]), (fused, deferred, k)
    # from normal_from_step on the term is in the step
    late = TD._run_trainer(dev, setup, True, True, with_depth=False, order=order, normal_weight=0.4,
                           normal_from_step=2, normal_alpha_min=ALPHA_MIN)
    assert late[0][:2] == off[0][:2] and late[0][2] > off[0][2]
    assert not torch.equal(late[1]["rotation"], off[1]["rotation"])


def _adam_allowances(raw_quats, g, t, lr, m1_scale, m2_scale):
    """What one first Adam step (moments from zero; BrushAdamConfig with rotation_grad_wrt_normalized) may differ by in
    the rotation block when the gradient at the normalised quaternion is known to +-t.  All [N,4] float64.
    The optimizer first maps v to the raw quaternion: v_raw = (I - n n^T) v / |q|, linear, so its allowance is
    sum_j |M_ij| t_j.  Moments: m1 = (1 - b1) v_raw, m2 = (1 - b2) v_raw^2.  Step: lr v_raw / (|v_raw| + eps) up to
    the bias corrections' roundings, a monotone function of v_raw bounded by 1 whose slope is at most
    1 / (|v_raw| + eps): a gradient that keeps its sign within +-t moves the step by lr t / (|v_raw| - t + eps), one
    that may change sign by up to 2 lr.  Each side rounds its few operations (16 U) and the final subtraction."""
    q = raw_quats.astype(np.float64)
    norm = np.sqrt((q * q).sum(1, keepdims=True))
    nrm = q / norm
    M = (np.eye(4)[None] - nrm[:, :, None] * nrm[:, None, :]) / norm[:, :, None]
    g_raw = np.einsum("nij,nj->ni", M, g)
    t_raw = np.einsum("nij,nj->ni", np.abs(M), t) * (1.0 + 16 * U) + 16 * U * np.einsum("nij,nj->ni", np.abs(M), np.abs(g))
    eps = 1e-15
    room = np.maximum(np.abs(g_raw) - t_raw, 0.0)
    d_step = lr * np.minimum(2.0, t_raw / (room + eps))
    tol_q = d_step * (1.0 + 16 * U) + 16 * U * lr + 2.0 * U * (np.abs(q) + lr)
    tol_m1 = m1_scale * t_raw * (1.0 + 4 * U) + 4 * U * m1_scale * np.abs(g_raw)
    tol_m2 = m2_scale * (2.0 * np.abs(g_raw) * t_raw + t_raw ** 2) * (1.0 + 8 * U) + 8 * U * m2_scale * g_raw ** 2
    return tol_q, tol_m1, tol_m2


@pytest.mark.parametrize("with_depth", [False, True])
def test_an_active_step_is_the_manual_composition(dev, deterministic, with_depth):
    """One step with the term on against the calls made by hand: forward with depth, colour loss, (brush_depth_loss,)
    brush_splat_normals, the feature replay, brush_normal_loss into v_pred, the loss word and the depth term's v_depth,
    the replay's transpose, the backward with depth, brush_splat_normals_backward, brush_adam_step.  With gt_depth the
    step's depth gradient is the sum of the two terms'."""
    import torch

    import brush_amd
    from brush_amd import _lib as L
    from brush_amd import render as R
    from brush_amd.depth_loss import depth_loss_into
    from brush_amd.features import feature_grads_from_aux, features_from_aux
    from brush_amd.normal_loss import normal_loss_into, splat_normals_backward_into, splat_normals_from
    from brush_amd.train import l1_ssim_loss

    setup = TD._trainer_setup(dev)
    mk, cams, gts, depths = setup
    kw = dict(normal_weight=0.4, normal_from_step=0, normal_alpha_min=ALPHA_MIN)
    if with_depth:
        kw.update(depth_weight=0.3)
    for fused in (True, False):  # an active term takes the separate-call path whatever fused_backward says
        got_losses, got = TD._run_trainer(dev, setup, fused, True, with_depth=with_depth, order=[1], **kw)
        s = mk()
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, depth_alpha_min=ALPHA_MIN, **kw)
        clock = brush_amd.SplatTrainer(mk(), cfg)
        n, ncoef = s.num_splats(), int(s.sh_coeffs.shape[1])
        m1, m2 = torch.zeros(n * (11 + 3 * ncoef), device=dev), torch.zeros(n * (11 + 3 * ncoef), device=dev)
        l, stream = L.lib(), torch.cuda.current_stream().cuda_stream
        means, log_scales, quats = s.means.detach(), s.log_scales.detach(), s.rotation.detach()
        sh, raw_opac = s.sh_coeffs.detach(), s.raw_opacity.detach()
        raw_quats0 = _np(quats).copy()
        norm_rot = torch.empty_like(quats)
        L.check(l.brush_normalize_quats(quats.data_ptr(), norm_rot.data_ptr(), n, stream), "normalize")
        bufs = R._depth_buffers(n, (W, Hh), dev)
        pred, aux, u = R._forward_impl(cams[1], (W, Hh), means, log_scales, norm_rot, sh, raw_opac, False, None,
                                       depth=bufs)
        loss, v_pred = l1_ssim_loss(pred, gts[1], cfg.ssim_weight, cfg.ssim_window_size, 1.0)
        colour_loss = float(loss)
        v_depth_d = None
        if with_depth:
            v_depth_d, _ = depth_loss_into(pred, bufs[0], depths[1], v_pred, weight=0.3, scale=0.001, offset=0.0,
                                           alpha_min=ALPHA_MIN, mode="depth", loss_accum=loss)
            only_depth = v_depth_d.clone()
        nimg = features_from_aux(u, aux, splat_normals_from(u, means, log_scales, norm_rot))
        v_depth, v_nimg, stats = normal_loss_into(u, pred, bufs[0], nimg, v_pred, weight=0.4, alpha_min=ALPHA_MIN,
                                                  loss_accum=loss, v_depth_accum=v_depth_d)
        assert 0.02 < float(stats[1]) < 0.98 and float(stats[0]) > 0 and float(loss) > colour_loss
        if with_depth:  # one v_depth: the sum of the two terms'
            alone, _, _ = normal_loss_into(u, pred, bufs[0], nimg, None, weight=0.4, alpha_min=ALPHA_MIN)
            assert v_depth is v_depth_d and torch.equal(v_depth, only_depth + alone)
            assert bool(alone.any()) and bool(only_depth.any())
        v_normals = torch.zeros((n, 3), device=dev)
        feature_grads_from_aux(u, aux, v_nimg, v_normals)
        g, _ = R._backward_impl(u, aux, means, log_scales, norm_rot, raw_opac, ncoef, pred, v_pred,
                                depth=(bufs[1], v_depth))
        splat_normals_backward_into(u, means, log_scales, norm_rot, v_normals, g["v_quats"])
        g_quats = _np(g["v_quats"]).astype(np.float64)
        tol_n = _transpose_allowance(u, aux, v_nimg, n, W, Hh, dev)
        tol_g = _through_vjp(u, means, log_scales, norm_rot, tol_n, dev)
        tol_g = tol_g + 2.0 * U * (np.abs(g_quats) + tol_g)
        acfg = L.BrushAdamConfig(clock._lr_mean(1.0), cfg.lr_scale, cfg.lr_rotation, cfg.lr_opac, cfg.lr_coeffs_dc,
                                 1.0 / cfg.lr_coeffs_sh_scale, 0.9, 0.999, 1e-15, 1, 1, 1.0)
        L.check(l.brush_adam_step(C.byref(acfg), n, R.sh_degree_from_coeffs(ncoef), means.data_ptr(),
                                  log_scales.data_ptr(), quats.data_ptr(), raw_opac.data_ptr(), sh.data_ptr(),
                                  g["v_means"].data_ptr(), g["v_scales"].data_ptr(), g["v_quats"].data_ptr(),
                                  g["v_opac"].data_ptr(), g["v_sh"].data_ptr(), m1.data_ptr(), m2.data_ptr(), stream),
                "adam")
        assert got_losses == [float(loss)], fused  # the loss to the bits
        for k, v in dict(means=means, log_scales=log_scales, raw_opacity=raw_opac, sh_coeffs=sh).items():
            assert np.array_equal(_bits(got[k]), _bits(v)), (fused, k)
        # the moments: [means 3N | log_scales 3N | quats 4N | raw_opac N | sh]: everything but the quaternion block
        qs = slice(6 * n, 10 * n)
        rest = np.ones(m1.numel(), bool)
        rest[qs] = False
        for name, m in (("moment1", m1), ("moment2", m2)):
            assert np.array_equal(_bits(got[name])[rest], _bits(m)[rest]), (fused, name)
        tol_q, tol_m1, tol_m2 = _adam_allowances(raw_quats0, g_quats, tol_g, cfg.lr_rotation, 1.0 - 0.9, 1.0 - 0.999)
        r = {"rotation": _ratio(got["rotation"], _np(quats).astype(np.float64), tol_q),
             "moment1": _ratio(got["moment1"][qs].view(n, 4), _np(m1)[qs].reshape(n, 4).astype(np.float64), tol_m1),
             "moment2": _ratio(got["moment2"][qs].view(n, 4), _np(m2)[qs].reshape(n, 4).astype(np.float64), tol_m2)}
        print(f"active step fused={fused} depth={with_depth}: rotation block |trainer - manual| / allowance", r)
        assert all(x <= 1.0 for x in r.values()), r
        assert not np.array_equal(_np(quats), raw_quats0)


def test_the_term_is_single_view_and_works_with_the_other_options(dev):
    import torch

    import brush_amd
    from brush_amd.pose import PoseTable

    setup = TD._trainer_setup(dev)
    mk, cams, gts, depths = setup
    kw = dict(normal_weight=0.4, normal_from_step=1, normal_alpha_min=ALPHA_MIN)
    s = mk()
    tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, **kw))
    tr.step(s, cams[0], gts[0], batch_views=2, grad_sync=lambda block, aux: None)  # before normal_from_step: allowed
    before = s.means.detach().clone()
    for extra in (dict(grad_sync=lambda block, aux: None), dict(exchange=object())):
        with pytest.raises(ValueError, match="the normal-consistency term is single-view"):
            tr.step(s, cams[0], gts[0], batch_views=2, **extra)
    assert torch.equal(s.means.detach(), before) and tr.iter == 1  # refused before anything was touched
    order = TD.ORDER[:6]
    kw["normal_from_step"] = 0
    for mode, extra in (("antialiased", dict(antialiased=True)), ("mcmc", dict(strategy="mcmc", mcmc_cap_max=512)),
                        ("poses", {})):
        poses = PoseTable(3, 1e-3, 1e-2, 1e-4) if mode == "poses" else None
        on = TD._run_trainer(dev, setup, True, True, False, order=order, poses=poses, **kw, **extra)
        assert np.isfinite(on[0]).all(), mode
        for k, v in on[1].items():
            assert bool(torch.isfinite(v).all()), (mode, k)
        poses2 = PoseTable(3, 1e-3, 1e-2, 1e-4) if mode == "poses" else None
        off = TD._run_trainer(dev, setup, True, True, False, order=order, poses=poses2, **extra)
        assert not torch.equal(on[1]["rotation"], off[1]["rotation"]), mode


# ---------------------------------------------------------------------------- 5. end to end
E2E_W = E2E_H = 96
E2E_WEIGHT = 0.05  # 2DGS's lambda_n: a hyper-parameter, not a measured number
E2E_STEPS = 300


def test_training_with_the_term_lowers_the_normal_disagreement(dev):
    """A 96x96 scene of 8 views of a known cloud of flat splats on a sphere, 1500 splats trained for 300 steps from the
    same seed with and without the term (weight 0.05 from step 0, no refinement).  Afterwards the mean over the
    training views of the loss at weight 1 (the mean over all pixels of alpha - Nr . Nd) must be strictly lower with the
    term: a comparison, not a threshold."""
    import torch

    import brush_amd
    from brush_amd.normal_loss import normal_loss_into

    w, h = E2E_W, E2E_H
    rng = np.random.default_rng(23)
    m = 1800
    dirs = rng.normal(size=(m, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    known = brush_amd.Splats.from_random_config(m, 0, (np.full(3, -0.8), np.full(3, 0.8)), rng, dev)
    with torch.no_grad():  # discs tangent to a sphere of radius 0.8: the z axis of each splat along its radius
        known.means.copy_(_tt((0.8 * dirs).astype(F), dev))
        zax = dirs
        xax = np.cross(zax, np.where(np.abs(zax[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
        xax /= np.linalg.norm(xax, axis=1, keepdims=True)
        yax = np.cross(zax, xax)
        Rm = np.stack([xax, yax, zax], axis=2)  # columns
        qw = np.sqrt(np.maximum(0.0, 1.0 + Rm[:, 0, 0] + Rm[:, 1, 1] + Rm[:, 2, 2])) / 2.0
        qx = np.copysign(np.sqrt(np.maximum(0.0, 1.0 + Rm[:, 0, 0] - Rm[:, 1, 1] - Rm[:, 2, 2])) / 2.0,
                         Rm[:, 2, 1] - Rm[:, 1, 2])
        qy = np.copysign(np.sqrt(np.maximum(0.0, 1.0 - Rm[:, 0, 0] + Rm[:, 1, 1] - Rm[:, 2, 2])) / 2.0,
                         Rm[:, 0, 2] - Rm[:, 2, 0])
        qz = np.copysign(np.sqrt(np.maximum(0.0, 1.0 - Rm[:, 0, 0] - Rm[:, 1, 1] + Rm[:, 2, 2])) / 2.0,
                         Rm[:, 1, 0] - Rm[:, 0, 1])
        known.rotation.copy_(_tt(np.stack([qw, qx, qy, qz], axis=1).astype(F), dev))
        known.log_scales.copy_(_tt(np.tile(np.log([0.07, 0.07, 0.007]), (m, 1)).astype(F), dev))
        known.raw_opacity.fill_(math.log(0.9 / 0.1))
    cams = [c for _, c in TL._ring_cameras(8, w, h, 4.0, 1.0, 0.1)]
    with torch.no_grad():
        gts = [known.render(cam, (w, h), False)[0][..., :3].clamp(0, 1).contiguous() for cam in cams]
    assert float(gts[0].max()) > 0.2

    def disagreement(splats):
        vals, fracs = [], []
        with torch.no_grad():
            for cam in cams:
                img, depth, nimg, aux = splats.render_normals(cam, (w, h))
                u = brush_amd.render.pack_uniforms(cam, (w, h), 0, 0)
                _, _, st = normal_loss_into(u, img, depth, nimg, None, weight=1.0, alpha_min=0.5)
                vals.append(float(st[0])), fracs.append(float(st[1]))
        return float(np.mean(vals)), float(np.mean(fracs))

    out = {}
    for name, weight in (("without", 0.0), ("with", E2E_WEIGHT)):
        splats = brush_amd.Splats.from_random_config(1500, 0, (np.full(3, -0.9), np.full(3, 0.9)),
                                                     np.random.default_rng(5), dev)
        cfg = brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, seed=7, total_steps=E2E_STEPS,
                                    normal_weight=weight, normal_from_step=0)
        tr = brush_amd.SplatTrainer(splats, cfg)
        order = np.random.default_rng(9).integers(0, len(cams), E2E_STEPS)
        losses = [tr.step(splats, cams[i], gts[i], 1.0)[0] for i in order]
        tr.sync(splats)
        assert bool(torch.isfinite(torch.cat(losses)).all()) and splats.num_splats() == 1500
        out[name] = disagreement(splats)
    print(f"normal disagreement at weight 1 after {E2E_STEPS} steps (mean l, valid fraction): without the term "
          f"{out['without']}, with weight {E2E_WEIGHT} {out['with']}")
    assert out["without"][1] > 0.02 and out["with"][1] > 0.02  # the measure looked at something
    assert out["with"][0] < out["without"][0]
