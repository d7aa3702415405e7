"""GPU checks of the camera-pose gradient (brush_render_backward_pose / brush_render_backward_adam_pose,
render_splats_pose, Splats.render_pose) and of per-view pose refinement in the trainer (brush_amd/pose.py,
TrainConfig.pose_opt, `python -m brush_amd.train_loop --pose-opt`).

Anchors: (1) nothing else moves; (2) the rigid identities between v_viewmat and the dense gradients of the same call,
within a rounding bound counted on the expression trees (pose_ref64.K_ROT / K_TR); (3) the float64 restatement
pose_ref64 on the CPU oracle's compact sums, at the project's gradient gate."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import aa_ref64 as A
from tests import helpers as H
from tests import pose_ref64 as P
from tests import test_gpu_antialias as TA
from tests import test_gpu_depth as TD
from tests import test_gpu_train_loop as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GRADS = ("v_means", "v_xy", "v_scales", "v_quats", "v_sh", "v_opac")
OMEGAS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.3, -0.5, 0.8]])
MARGINS = {}


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd  # noqa: F401

    yield torch.device("cuda:0")
    write_margins()


def write_margins():
    """The achieved worst ratios against the oracle gate and the identity bounds, folded into the file's entries (this
    module and tests/test_gpu_general_camera.py both record here, and either may run alone)."""
    if not MARGINS:
        return
    path = os.environ.get("BRUSH_POSE_MARGINS") or os.path.join(ROOT, "profiles", "pose_margins.json")
    try:
        try:
            with open(path) as f:
                merged = json.load(f)
        except (OSError, ValueError):
            merged = {}
        merged.update(MARGINS)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
    except OSError as e:  # a read-only checkout: never turn a finished run red from here
        print(f"pose margins not written: {e!r}")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


@functools.lru_cache(maxsize=None)
def _scene(kind):
    """test_gpu_depth's scenes, the quaternions normalised in f32 (what Splats.render feeds the op)."""
    cloud, w, h = TD._scene(kind)
    cloud = dict(cloud)
    q = np.asarray(cloud["quats"], np.float32)
    cloud["quats"] = (q / np.sqrt((q * q).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return cloud, w, h


_np = TD._np


def _call(dev, cloud, w, h, det, aa=False, v_out=None, v_d=None, pose=True, viewmat=None, camera=None):
    """One forward (with the depth map when v_d is given) and one backward through the C ABI.  Returns (img, aux, u,
    dense gradients as numpy, v_viewmat [3,4] float32 or None).  `camera`: a brush_amd.Camera in place of the reference
    test camera."""
    import torch

    from brush_amd import render as R

    t = TD._tensors(cloud, dev)
    n = cloud["means"].shape[0]
    bufs = R._depth_buffers(n, (w, h), dev) if v_d is not None else None
    img, aux, u = R._forward_impl(camera or TD._camera(w, h), (w, h), t["means"], t["log_scales"], t["quats"],
                                  t["sh"], t["raw_opac"], False, None, deterministic=det, depth=bufs, antialiased=aa,
                                  viewmat=viewmat)
    pb = R.pose_buffers(n, dev) if pose else None
    if pb is not None:
        pb[0].fill_(float("nan"))
    g, _ = R._backward_impl(u, aux, t["means"], t["log_scales"], t["quats"], t["raw_opac"], cloud["sh"].shape[1], img,
                            v_out, depth=None if v_d is None else (bufs[1], v_d), pose=pb)
    torch.cuda.synchronize()
    return img, aux, u, {k: _np(g[k]) for k in GRADS}, (None if pb is None else _np(pb[0]).reshape(3, 4))


def _compact_sums(aux, n):
    """The default mode's compact-order accumulators after a backward (common.hpp: [v_xy 2 | v_conic 3 | v_rgb 3 |
    v_alpha | v_z ...] per visible splat, at the start of the backward's workspace): a scale for the bounds."""
    V = aux.read_num_visible()
    rows = _np(aux.bwd_ws[: max(n, 1) * 64].view(dtype=__import__("torch").float32)).reshape(-1, 16)[:V]
    gid = _np(aux.global_from_compact_gid[:V]).astype(np.int64)
    return V, gid, rows.astype(np.float64)


# ---------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("kind", ["basic_case", "ragged", "c1"])
def test_dense_gradients_bitwise_unchanged(dev, kind, aa, depth):
    cloud, w, h = _scene(kind)
    v_out, v_d = TD._upstream(dev, w, h, seed=5)
    v_d = v_d if depth else None
    i0, a0, _, g0, _ = _call(dev, cloud, w, h, True, aa, v_out, v_d, pose=False)
    i1, a1, _, g1, vv = _call(dev, cloud, w, h, True, aa, v_out, v_d, pose=True)
    assert _np(i0).tobytes() == _np(i1).tobytes()
    for k in GRADS:
        assert g0[k].tobytes() == g1[k].tobytes(), k
    assert np.isfinite(vv).all() and np.abs(vv).max() > 0
    # the default mode too, where the dense arrays are not bitwise repeatable: the pose kernels only read
    _, _, _, g2, _ = _call(dev, cloud, w, h, False, aa, v_out, v_d, pose=True)
    for k in GRADS:
        scale = float(np.abs(g0[k]).max())
        ok, err, bad = H.all_close_report(g2[k], g0[k], 1e-3, 1e-4 * scale + 1e-12)
        assert ok, (k, err, bad)


# ---------------------------------------------------------------------------- 2. rigid identities
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "empty", "c1", "S1"])
def test_rigid_identities_from_the_calls_own_outputs(dev, kind, det, aa):
    """pose_ref64: K_ROT / K_TR and the identities.  The bound's scale comes from the compact sums of a default-mode
    call on the same inputs (the deterministic mode keeps them in pieces), read back from its workspace."""
    check_rigid_identities(dev, kind, det, aa, *_scene(kind))


def check_rigid_identities(dev, kind, det, aa, cloud, w, h, camera=None):
    """The body of test_rigid_identities_from_the_calls_own_outputs; `kind` names the scene (and the camera) in the
    recorded margins."""
    n = cloud["means"].shape[0]
    v_out, v_d = TD._upstream(dev, w, h, seed=11)
    for depth in (None, v_d):
        _, aux, u, g, vv = _call(dev, cloud, w, h, det, aa, v_out, depth, camera=camera)
        if det:
            _, aux_s, _, _, _ = _call(dev, cloud, w, h, False, aa, v_out, depth, camera=camera)
        else:
            aux_s = aux
        V, gid, rows = _compact_sums(aux_s, n)
        un = P.uniforms_ns(u)
        v_z = rows[:, 9] if depth is not None else None
        v_comp = rows[:, 8] * A.sigmoid64(cloud["raw_opac"][gid]) if aa else None
        lhs_r, rhs_r, lhs_t, rhs_t = P.identity_sides(un, cloud["means"], cloud["quats"], vv, g["v_means"], g["v_quats"],
                                                      OMEGAS)
        mag_r, mag_t = P.identity_mags(un, cloud["means"], cloud["log_scales"], cloud["quats"], rows[:, 0:2],
                                       rows[:, 2:5], OMEGAS, v_z=v_z, v_comp=v_comp, gids=gid)
        if kind == "empty":
            assert V == 0 and not vv.any()
        er, et = np.abs(lhs_r - rhs_r), np.abs(lhs_t - rhs_t)
        br, bt = P.K_ROT * U * mag_r, P.K_TR * U * mag_t
        tag = f"{kind} det={det} aa={aa} depth={depth is not None}"
        rr = float((er / np.maximum(br, 1e-300)).max()) if V else 0.0
        rt = float((et / np.maximum(bt, 1e-300)).max()) if V else 0.0
        print(f"[{tag}] V={V} rotation |lhs-rhs| {er} bound {br} (lhs {lhs_r}); translation {et} bound {bt} "
              f"(lhs {lhs_t}); worst ratios {rr:.3f} {rt:.3f}")
        MARGINS[f"identity/{tag}"] = {"rotation": rr, "translation": rt}
        assert (er <= br + 1e-300).all(), (tag, er, br)
        assert (et <= bt + 1e-300).all(), (tag, et, bt)
        if V:
            assert (np.abs(lhs_r) > br).any() and (np.abs(lhs_t) > bt).any(), tag  # the identities are resolved


# ---------------------------------------------------------------------------- 3. against the reference
def _oracle_sums(ud, cloud, v_out_np):
    o_img, o_aux = O.render_forward(ud, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                    cloud["raw_opac"])
    g = O.render_backward(ud, o_aux, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["raw_opac"], o_img,
                          v_out_np)
    V = int(o_aux["num_visible"][0])
    return g, V, o_aux["global_from_compact_gid"][:V].astype(np.int64)


def _gate(tag, got, want, mag, record=True):
    """The project's gradient gate: rtol 1e-3, atol 1e-4 mag, mag the sum of absolute terms of each entry.  `record`:
    False for a control against a deliberately wrong reference, whose ratio is no margin."""
    err = np.abs(got.astype(np.float64) - want)
    allow = 1e-3 * np.abs(want) + 1e-4 * mag + 1e-30
    ratio = float((err / allow).max())
    print(f"[{tag}] max|gpu - ref| {err.max():.3e} worst ratio to the gate {ratio:.3f}\n got {got}\n want {want}")
    if record:
        MARGINS[f"oracle/{tag}"] = ratio
    assert (err <= allow).all(), (tag, err, allow)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("kind", ["tiny_case", "basic_case", "ragged", "c1"])
def test_against_pose_ref64_on_the_oracle(dev, kind, det):
    check_against_pose_ref64(dev, kind, det, *_scene(kind))


LEGS = ("plain", "depth", "antialiased")


def check_against_pose_ref64(dev, kind, det, cloud, w, h, camera=None, mutate=None, legs=LEGS):
    """The body of test_against_pose_ref64_on_the_oracle; `kind` names the scene (and the camera) in the recorded
    margins.  `mutate`: one of pose_ref64.MUTATIONS, for the negative controls (nothing is recorded then); `legs`: the
    legs to run."""
    from brush_amd.render import uniforms_to_numpy

    v_out, v_d = TD._upstream(dev, w, h, seed=6)
    rec = mutate is None
    # plain
    _, aux, u, g, vv = _call(dev, cloud, w, h, det, False, v_out, camera=camera)
    ud, un = uniforms_to_numpy(aux), P.uniforms_ns(u)
    base, V, gid = _oracle_sums(ud, cloud, _np(v_out))
    assert V == aux.read_num_visible()
    want, mag = P.pose_grad64(un, cloud["means"], cloud["log_scales"], cloud["quats"], base["v_xy_local"][:V],
                              base["v_conics"][:V], gids=gid, mutate=mutate)
    if "plain" in legs:
        _gate(f"{kind} det={det} plain", vv, want, mag, rec)
    # with a depth gradient: the depth-as-colour twin of test_gpu_depth.py adds its (v_xy, v_conic) and brings v_z
    _, aux_d, _, _, vv_d = _call(dev, cloud, w, h, det, False, v_out, v_d, camera=camera)
    tw, _ = TD._twin(cloud, u)
    vt = np.zeros((h, w, 4), np.float32)
    vt[..., 0] = _np(v_d)
    twin, Vt, gid_t = _oracle_sums(ud | {"sh_degree": 0}, tw, vt)
    assert Vt == V and np.array_equal(gid_t, gid)
    v_z = twin["v_sh"][gid, 0, 0].astype(np.float64) / float(TD.C0)
    want, mag = P.pose_grad64(un, cloud["means"], cloud["log_scales"], cloud["quats"],
                              base["v_xy_local"][:V].astype(np.float64) + twin["v_xy_local"][:V],
                              base["v_conics"][:V].astype(np.float64) + twin["v_conics"][:V], v_z=v_z, gids=gid,
                              mutate=mutate)
    if "depth" in legs:
        _gate(f"{kind} det={det} depth", vv_d, want, mag, rec)
    # antialiased: the opacity twin of test_gpu_antialias.py; dL/do of the twin's raw opacity carries v_comp
    _, aux_a, _, _, vv_a = _call(dev, cloud, w, h, det, True, v_out, camera=camera)
    ta = TA._twin(cloud, aux_a)
    tb, Va, gid_a = _oracle_sums(uniforms_to_numpy(aux_a), ta, _np(v_out))
    assert Va == aux_a.read_num_visible()
    ot = A.sigmoid64(ta["raw_opac"][gid_a])
    dd = ot * (1.0 - ot)
    dldo = np.where(dd > 0, tb["v_opac"][gid_a].astype(np.float64) / np.where(dd > 0, dd, 1.0), 0.0)
    want, mag = P.pose_grad64(un, cloud["means"], cloud["log_scales"], cloud["quats"], tb["v_xy_local"][:Va],
                              tb["v_conics"][:Va], v_comp=dldo * A.sigmoid64(cloud["raw_opac"][gid_a]), gids=gid_a,
                              mutate=mutate)
    if "antialiased" in legs:
        _gate(f"{kind} det={det} antialiased", vv_a, want, mag, rec)


# ---------------------------------------------------------------------------- 4. deterministic mode, capture
def test_deterministic_repeats_and_survives_graph_capture(dev):
    import torch

    from brush_amd import render as R

    cloud, w, h = _scene("c1")
    v_out, v_d = TD._upstream(dev, w, h, seed=7)
    a = _call(dev, cloud, w, h, True, False, v_out, v_d)[4]
    b = _call(dev, cloud, w, h, True, False, v_out, v_d)[4]
    assert a.tobytes() == b.tobytes() and np.abs(a).max() > 0

    cloud, w, h = _scene("ragged")
    v_out, v_d = TD._upstream(dev, w, h, seed=8)
    t = TD._tensors(cloud, dev)
    n = cloud["means"].shape[0]
    cam = TD._camera(w, h)

    def step():
        bufs = R._depth_buffers(n, (w, h), dev)
        img, aux, u = R._forward_impl(cam, (w, h), t["means"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"],
                                      False, None, deterministic=True, depth=bufs)
        pb = R.pose_buffers(n, dev)
        g, _ = R._backward_impl(u, aux, t["means"], t["log_scales"], t["quats"], t["raw_opac"], cloud["sh"].shape[1],
                                img, v_out, depth=(bufs[1], v_d), pose=pb)
        return [pb[0], g["v_means"]]

    eager = [x.clone() for x in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the capture stream
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # and the call does not synchronise
    try:
        with torch.cuda.stream(s):
            step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = step()
    for o in outs:
        o.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, outs):
        assert _np(x).tobytes() == _np(y).tobytes()


# ---------------------------------------------------------------------------- 5. edge cases
def test_empty_scene_and_no_splats_give_twelve_zeros(dev):
    import torch

    from brush_amd import _lib
    from brush_amd import render as R

    cloud, w, h = _scene("empty")
    v_out, _ = TD._upstream(dev, w, h, seed=2)
    for det in (False, True):
        vv = _call(dev, cloud, w, h, det, False, v_out)[4]
        assert vv.tobytes() == np.zeros((3, 4), np.float32).tobytes()
    zero = {k: v[:0] for k, v in cloud.items()}
    vv = _call(dev, zero, w, h, False, False, v_out)[4]
    assert vv.tobytes() == np.zeros((3, 4), np.float32).tobytes()

    # a too-small pose workspace is refused before any launch
    cloud, w, h = _scene("basic_case")
    t = TD._tensors(cloud, dev)
    n = cloud["means"].shape[0]
    img, aux, u = R._forward_impl(TD._camera(w, h), (w, h), t["means"], t["log_scales"], t["quats"], t["sh"],
                                  t["raw_opac"], False, None)
    l = _lib.lib()
    nb = C.c_size_t()
    _lib.check(l.brush_bwd_workspace_size_flags(n, w, h, int(u.sh_degree), int(aux.max_intersects), aux.workspace_flags,
                                                C.byref(nb)), "size")
    ws, s = aux.backward_workspace(nb.value, dev)
    pb = R.pose_buffers(n, dev)
    gb = [torch.zeros(n * k, device=dev) for k in (3, 2, 3, 4, cloud["sh"].shape[1] * 3, 1)]
    v_out, _ = TD._upstream(dev, w, h, seed=2)
    args = [C.byref(u), C.byref(s), t["means"].data_ptr(), t["log_scales"].data_ptr(), t["quats"].data_ptr(),
            t["raw_opac"].data_ptr(), n, img.data_ptr(), v_out.data_ptr(), None, None] + [b.data_ptr() for b in gb] + \
           [ws.data_ptr(), nb.value]
    stream = torch.cuda.current_stream().cuda_stream
    assert l.brush_render_backward_pose(*args, pb[0].data_ptr(), pb[1].data_ptr(), pb[1].numel() - 1, stream) == -2
    assert l.brush_render_backward_pose(*args, None, pb[1].data_ptr(), pb[1].numel(), stream) == -1
    assert l.brush_render_backward_pose(*args, pb[0].data_ptr(), pb[1].data_ptr(), pb[1].numel(), stream) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 6. autograd
def test_autograd_op_matches_the_abi_and_reaches_delta(dev):
    import torch

    import brush_amd
    from brush_amd.pose import apply_delta

    cloud, w, h = _scene("ragged")
    cam = TD._camera(w, h)
    v_out, v_d = TD._upstream(dev, w, h, seed=4)
    M0 = torch.from_numpy(cam.world_to_local())
    for depth in (False, True):
        t = TD._tensors(cloud, dev, grad=True)
        vm = M0.clone().requires_grad_(True)
        res = brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), vm, deterministic=True, depth=depth)
        outs, gos = ([res[0], res[1]], [v_out, v_d]) if depth else ([res[0]], [v_out])
        ps = [t["means"], t["xy"], t["log_scales"], t["quats"], t["sh"], t["raw_opac"], vm]
        gr = torch.autograd.grad(outs, ps, gos)
        img0, _, _, g0, vv = _call(dev, cloud, w, h, True, False, v_out, v_d if depth else None)
        assert _np(res[0]).tobytes() == _np(img0).tobytes()  # the camera's own matrix: the bits of render_splats
        for k, x in zip(GRADS, gr[:6]):
            assert _np(x).tobytes() == g0[k].tobytes(), k
        gv = gr[6]
        assert gv.device.type == "cpu" and gv.shape == (4, 4) and gv.dtype == torch.float32
        assert gv[:3].numpy().tobytes() == vv.tobytes() and not gv[3].any()
    # untracked: plain forward, same image
    with torch.no_grad():
        t = TD._tensors(cloud, dev)
        img, aux = brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), M0)
        ref, _ = brush_amd.render_splats(cam, (w, h), *TD._args(t))
    assert _np(img).tobytes() == _np(ref).tobytes()
    # down to a twist through apply_delta, with only the pose tracked
    delta = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    img, _ = brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), apply_delta(M0, delta).to(torch.float32),
                                          deterministic=True)
    (img * v_out).sum().backward()
    gp = torch.from_numpy(_call(dev, cloud, w, h, True, False, v_out)[4].astype(np.float64))
    want = torch.zeros(6, dtype=torch.float64)
    for j in range(6):  # d exp(delta) M0 / d delta_j at 0 is the generator X_j M0
        want[j] = ((torch.from_numpy(P.twist_matrix(np.eye(6)[j])) @ M0.double())[:3] * gp).sum()
    assert torch.allclose(delta.grad, want, rtol=1e-6, atol=1e-9 * float(want.abs().max())), (delta.grad, want)
    # a device matrix is refused
    with pytest.raises(ValueError, match="CPU tensor"):
        brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), M0.to(dev))
    # Splats.render_pose is the same op
    splats = brush_amd.Splats(*(torch.as_tensor(cloud[k], device=dev)
                                for k in ("means", "sh", "quats", "raw_opac", "log_scales")))
    with torch.no_grad():
        a, _ = splats.render_pose(cam, (w, h), M0)
        b, _ = splats.render(cam, (w, h))
    assert _np(a).tobytes() == _np(b).tobytes()


# ---------------------------------------------------------------------------- 7. pose fit
def test_pose_fit_recovers_a_perturbed_camera(dev):
    """The run tests/test_pose_cpu.py rehearses on the oracle (same scene, perturbation, learning rates and steps:
    pose_ref64.FIT_*), here through render_splats_pose: it must end below one tenth of its initial rotation and
    translation error."""
    check_pose_fit(dev, P.fit_problem(), TD._camera(P.FIT_W, P.FIT_H), "pose_fit")


def check_pose_fit(dev, cloud, cam, key):
    """The body of test_pose_fit_recovers_a_perturbed_camera for the fit cloud in front of `cam`; `key` names the
    recorded margins."""
    import torch

    import brush_amd

    w, h = P.FIT_W, P.FIT_H
    t = TD._tensors(cloud, dev)
    M_true = cam.world_to_local().astype(np.float64)
    with torch.no_grad():
        target, _ = brush_amd.render_splats(cam, (w, h), *TD._args(t))

    def loss_fn(viewmat):
        img, _ = brush_amd.render_splats_pose(cam, (w, h), *TD._args(t), viewmat, deterministic=True)
        return 0.5 * ((img - target) ** 2).sum() / float(w * h)

    first, last, losses = P.fit_pose(loss_fn, M_true)
    print(f"rotation {first[0]:.4f} -> {last[0]:.5f} rad, translation {first[1]:.4f} -> {last[1]:.5f}; "
          f"loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    MARGINS[key] = {"rotation": [first[0], last[0]], "translation": [first[1], last[1]]}
    assert last[0] < 0.1 * first[0] and last[1] < 0.1 * first[1], (first, last)


# ---------------------------------------------------------------------------- 8. trainer
def _trainer_cloud():
    cloud = H.synthetic_cloud(4096, 3, seed=13, mean_mult=0.0005)
    cloud["log_scales"] = cloud["log_scales"] - 3.0
    return cloud


def _bits(splats, tr):
    return ({k: _np(getattr(splats, k)).tobytes() for k in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")},
            _np(tr.moment1).tobytes(), _np(tr.moment2).tobytes())


def test_trainer_paths_hold_the_same_deltas_and_splats(dev, deterministic):
    """Five deterministic steps over three views with poses: the fused eager, fused deferred-SH and separate-call
    paths leave the same bits in the splats, the moments and the twists; the run repeats bitwise; and the option off is
    today's trajectory (compared with a run in a process that never imports brush_amd.pose)."""
    import torch

    import brush_amd
    from brush_amd.pose import PoseTable

    cloud = _trainer_cloud()
    w, h = 128, 80
    cams = [c for _, c in TL._ring_cameras(3, w, h, 8.0, 1.0, 0.3)]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda: brush_amd.Splats(tt(cloud["means"]), tt(cloud["sh"]), tt(cloud["quats"] * 1.7), tt(cloud["raw_opac"]),
                                  tt(cloud["log_scales"]))
    torch.manual_seed(5)
    gts = [torch.rand((h, w, 3), device=dev) for _ in cams]
    order = [0, 1, 1, 2, 0, 1, 2, 2]  # back-to-back repeats included

    def run(fused, deferred, with_poses=True):
        s = mk()
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0,
                                                             deferred_sh_adam=deferred))
        tr.fused_backward = fused
        poses = PoseTable(len(cams), 1e-3, 1e-2, 1e-4) if with_poses else None
        losses = []
        for i in order:
            kw = dict(view_index=i, poses=poses) if with_poses else {}
            losses.append(float(tr.step(s, cams[i], gts[i], **kw)[0]))
        tr.sync(s)
        if poses is not None:
            poses.apply_all()
        return losses, _bits(s, tr), (None if poses is None else poses.delta.numpy().tobytes()), poses

    runs = [run(True, False), run(True, True), run(False, False), run(True, True)]
    for r in runs[1:]:
        assert r[:3] == runs[0][:3]
    poses = runs[0][3]
    assert poses.steps == [order.count(i) for i in range(3)] and bool(poses.delta.abs().sum() > 0)
    # with the option off nothing changes: the same calls as a process without brush_amd.pose
    off = run(True, True, with_poses=False)
    assert off[0] != runs[0][0]  # the poses moved the trajectory
    code = (
        "import sys, json, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "import brush_amd\n"
        "from brush_amd import render as R\n"
        "from tests import test_gpu_pose as T\n" % ROOT
    )
    # (the child imports this module for the scene only; brush_amd.pose stays unloaded, asserted below)
    code += (
        "R.DETERMINISTIC = True\n"
        "dev = torch.device('cuda:0')\n"
        "cloud = T._trainer_cloud(); w, h = 128, 80\n"
        "cams = [c for _, c in T.TL._ring_cameras(3, w, h, 8.0, 1.0, 0.3)]\n"
        "tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)\n"
        "s = brush_amd.Splats(tt(cloud['means']), tt(cloud['sh']), tt(cloud['quats'] * 1.7), tt(cloud['raw_opac']), tt(cloud['log_scales']))\n"
        "torch.manual_seed(5)\n"
        "gts = [torch.rand((h, w, 3), device=dev) for _ in cams]\n"
        "tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, deferred_sh_adam=True))\n"
        "losses = [float(tr.step(s, cams[i], gts[i])[0]) for i in %r]\n"
        "tr.sync(s)\n"
        "assert 'brush_amd.pose' not in sys.modules\n"
        "import hashlib\n"
        "print(json.dumps({'losses': losses, 'hash': hashlib.sha256(b''.join(T._bits(s, tr)[0].values())).hexdigest()}))\n"
        % (order,)
    )
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    import hashlib

    assert child["losses"] == off[0]
    assert child["hash"] == hashlib.sha256(b"".join(off[1][0].values())).hexdigest()
    # pose refinement is single-view
    s = mk()
    tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0))
    with pytest.raises(ValueError, match="single-view"):
        tr.step(s, cams[0], gts[0], grad_sync=lambda b, a: None, view_index=0, poses=PoseTable(3, 1e-3, 1e-2))
    with pytest.raises(ValueError, match="view_index"):
        tr.step(s, cams[0], gts[0], poses=PoseTable(3, 1e-3, 1e-2))


def test_trainer_pushes_the_abi_gradient(dev, deterministic):
    """One trainer step with poses: the twelve words it pushes are those of brush_render_backward_pose on the same
    forward and upstream gradient, on all three paths."""
    import torch

    import brush_amd
    from brush_amd import render as R
    from brush_amd.pose import PoseTable
    from brush_amd.train import l1_ssim_loss

    cloud = _trainer_cloud()
    w, h = 128, 80
    cam = TL._ring_cameras(3, w, h, 8.0, 1.0, 0.3)[0][1]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q = cloud["quats"] / np.linalg.norm(cloud["quats"], axis=1, keepdims=True)
    torch.manual_seed(5)
    gt = torch.rand((h, w, 3), device=dev)
    n = cloud["means"].shape[0]
    pushed = []
    for fused, deferred in ((True, False), (True, True), (False, False)):
        s = brush_amd.Splats(tt(cloud["means"]), tt(cloud["sh"]), tt(q.astype(np.float32)), tt(cloud["raw_opac"]),
                             tt(cloud["log_scales"]))
        before = {k: getattr(s, k).detach().clone() for k in ("means", "log_scales", "rotation", "sh_coeffs", "raw_opacity")}
        tr = brush_amd.SplatTrainer(s, brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, deferred_sh_adam=deferred))
        tr.fused_backward = fused
        poses = PoseTable(1, 1e-3, 1e-2)
        tr.step(s, cam, gt, view_index=0, poses=poses)
        torch.cuda.synchronize()
        pushed.append(poses._slot(0).numpy().copy())
    nr = torch.empty_like(before["rotation"])
    from brush_amd import _lib

    _lib.check(_lib.lib().brush_normalize_quats(before["rotation"].data_ptr(), nr.data_ptr(), n,
                                                torch.cuda.current_stream().cuda_stream), "brush_normalize_quats")
    img, aux, u = R._forward_impl(cam, (w, h), before["means"], before["log_scales"], nr, before["sh_coeffs"],
                                  before["raw_opacity"], False, None, viewmat=cam.world_to_local())
    _, v_pred = l1_ssim_loss(img, gt, 0.2, 11, 1.0)
    pb = R.pose_buffers(n, dev)
    R._backward_impl(u, aux, before["means"], before["log_scales"], nr, before["raw_opacity"], cloud["sh"].shape[1], img,
                     v_pred, pose=pb)
    want = _np(pb[0])
    assert np.abs(want).max() > 0
    for p in pushed:
        assert p.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------- 9. end to end
POSE_NOISE = (0.02, 0.05)   # per-view pose noise of the end-to-end scene: rotation [rad], translation [world units]
E2E_STEPS = 4000


class _NoisyCamera:
    """A dataset camera whose world-to-camera matrix carries a fixed camera-frame twist (COLMAP-like pose error)."""

    def __init__(self, cam, delta):
        self._cam, self._delta = cam, np.asarray(delta, np.float64)
        for k in ("position", "rotation", "fov_x", "fov_y", "center_uv"):
            setattr(self, k, getattr(cam, k))

    def focal(self, img_size):
        return self._cam.focal(img_size)

    def center(self, img_size):
        return self._cam.center(img_size)

    def local_to_world(self):
        return np.linalg.inv(self.world_to_local().astype(np.float64))

    def world_to_local(self):
        return (P.expm_series(P.twist_matrix(self._delta)) @ self._cam.world_to_local().astype(np.float64)).astype(np.float32)


def _centre(M):
    M = np.asarray(M, np.float64)
    return -M[:3, :3].T @ M[:3, 3]


def _perturb(data, seed=3):
    rng = np.random.default_rng(seed)
    true = [v.camera.world_to_local().astype(np.float64) for v in data.train.views]
    for v in data.train.views:
        d = np.concatenate([rng.normal(size=3) * POSE_NOISE[0], rng.normal(size=3) * POSE_NOISE[1]])
        v.camera = _NoisyCamera(v.camera, d)
    return true


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    return TL._write_scene(str(tmp_path_factory.mktemp("pose_scene")), dev)


def test_pose_refinement_end_to_end(dev, scene_dir, deterministic):
    """The scene of test_gpu_train_loop.py with its training poses perturbed (POSE_NOISE): without refinement the run
    loses PSNR against clean poses; with TrainConfig.pose_opt the final loss is lower than without and the training
    cameras' centres end closer to the true ones than they started.  (Eval views keep their true poses, and the
    refined scene is free to settle in a slightly moved frame: the eval PSNR with the option on is reported, the
    assertion is on the training loss and the camera centres.)
    Measured on the MI355X (4000 steps, noise 0.02 rad / 0.05 units, the default learning rates): eval PSNR 42.1 dB
    with clean poses, 15.2 dB noisy without refinement, 25.9 dB with it; mean camera-centre error
    0.083 -> 0.070, mean rotation error 0.035 -> 0.017 rad.  A translation learning rate of 2e-3 and more lets the
    centres wander (0.083 -> 0.12) while the loss still falls: panning and translating are hard to tell apart here."""
    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop, load_dataset

    def run(noisy, pose_opt):
        data, _ = load_dataset(scene_dir)
        true = _perturb(data) if noisy else None
        cfg = TrainConfig(warmup_steps=50, refine_every=50, pose_opt=pose_opt)
        loop = TrainLoop(data, cfg, steps=E2E_STEPS, init_count=2000, sh_degree=3, seed=5)
        start = [m for _, m in loop.train_viewmats()]
        for _ in range(E2E_STEPS):
            loop.step()
        row, _ = loop.evaluate()
        _, log = loop.finish()
        end = [m for _, m in loop.train_viewmats()]
        return dict(psnr=row.psnr, loss=float(np.mean(log.losses[-100:])), log=log, true=true, start=start, end=end)

    clean, off, on = run(False, False), run(True, False), run(True, True)
    err = lambda ms, true: float(np.mean([np.linalg.norm(_centre(m) - _centre(t)) for m, t in zip(ms, true)]))
    e0, e1 = err(on["start"], on["true"]), err(on["end"], on["true"])
    print(f"pose e2e: eval psnr clean {clean['psnr']:.3f} noisy/off {off['psnr']:.3f} noisy/on {on['psnr']:.3f}; "
          f"final loss clean {clean['loss']:.5f} off {off['loss']:.5f} on {on['loss']:.5f}; "
          f"mean camera-centre error {e0:.4f} -> {e1:.4f}")
    MARGINS["e2e"] = {"psnr": [clean["psnr"], off["psnr"], on["psnr"]], "loss": [clean["loss"], off["loss"], on["loss"]],
                      "centre_error": [e0, e1]}
    assert off["psnr"] < clean["psnr"] - 0.5          # the noise visibly costs PSNR
    assert on["loss"] < off["loss"]
    assert e1 < e0
    assert on["log"].pose_opt and len(on["log"].pose_deltas) == 16 and not off["log"].pose_opt
    assert off["log"].pose_deltas is None and [m.tobytes() for m in off["start"]] == [m.tobytes() for m in off["end"]]


def test_cli_writes_cameras_and_log_fields(scene_dir, tmp_path):
    out_json, cams = str(tmp_path / "log.json"), str(tmp_path / "cams.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "60", "--init-count", "1000",
                        "--pose-opt", "--export-cameras", cams, "--json", out_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_json) as f:
        log = json.load(f)
    assert log["pose_opt"] is True and len(log["pose_deltas"]) == 16 and len(log["pose_deltas"][0]) == 6
    assert any(any(x != 0.0 for x in d) for d in log["pose_deltas"])
    with open(cams) as f:
        cj = json.load(f)
    assert cj["pose_opt"] is True and len(cj["cameras"]) == 16
    for c in cj["cameras"]:
        M = np.array(c["world_to_camera"])
        assert isinstance(c["name"], str) and M.shape == (4, 4) and np.allclose(M[3], [0, 0, 0, 1])
        assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-5
