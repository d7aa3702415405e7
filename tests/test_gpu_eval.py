"""GPU checks of the evaluation path: brush_eval_metrics against a float64 restatement of eval.rs + ssim.rs (the 2-D
window of ssim.rs:36-40 as a grouped conv2d, not the kernel's separable form), its edge semantics, determinism and
graph capture, file -> cameras -> pixels -> metrics end to end for a PLY on NeRF-synthetic and COLMAP datasets (cameras
built by hand from the files, images rendered by the oracle), the trainer's state across an eval, and its speed."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as E
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ref_metrics(pred_rgb, gt_rgb, window=11):
    """(mse, psnr, ssim) in float64 on the CPU: eval.rs:55-59 and ssim.rs:34-101 with Ssim::new(window, 3)."""
    import torch
    import torch.nn.functional as F

    x = torch.as_tensor(np.asarray(pred_rgb, dtype=np.float64))
    y = torch.as_tensor(np.asarray(gt_rgb, dtype=np.float64))
    mse = float(((x - y) ** 2).mean())
    psnr = math.log(1.0 / mse) * 10.0 / math.log(10.0) if mse > 0 else math.inf
    g = torch.tensor([math.exp(-((i - window // 2) ** 2) / (2.0 * 1.5 ** 2)) for i in range(window)],
                     dtype=torch.float64)
    g = g / g.sum()
    w2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
    x, y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    blur = lambda t: F.conv2d(t, w2, None, stride=1, padding=-(-window // 2), groups=3)  # div_ceil, ssim.rs:49
    mu_x, mu_y = blur(x), blur(y)
    s_xx = (blur(x * x) - mu_x * mu_x).clamp_min(0)
    s_yy = (blur(y * y) - mu_y * mu_y).clamp_min(0)
    s_xy = blur(x * y) - mu_x * mu_y
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((mu_x * mu_y * 2 + c1) * (s_xy * 2 + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_xx + s_yy + c2))
    assert m.shape[-2:] == (pred_rgb.shape[0] + 2, pred_rgb.shape[1] + 2)
    return mse, psnr, float(m.mean())


def _inputs(w, h, c, u8, seed):
    """Random pred [h,w,4] f32 and a partly correlated gt [h,w,c] (u8 or f32), both numpy."""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3))
    pred = np.concatenate([base * 0.8 + rng.random((h, w, 3)) * 0.2, rng.random((h, w, 1))], 2).astype(np.float32)
    gt = np.clip(base * 0.7 + rng.random((h, w, 3)) * 0.3, 0.0, 1.0)
    if c == 4:
        gt = np.concatenate([gt, rng.random((h, w, 1))], 2)
    gt = (gt * 255.0).round().astype(np.uint8) if u8 else gt.astype(np.float32)
    return pred, gt


def _gt_f32(gt):
    """What the kernel reads: u8 / 255 as an IEEE f32 division (image_to_tensor), f32 as is."""
    return gt.astype(np.float32) / np.float32(255.0) if gt.dtype == np.uint8 else gt


def _check(got, pred, gt, window):
    mse, psnr, ssim = ref_metrics(pred[..., :3], _gt_f32(gt)[..., :3], window)
    g_mse, g_psnr, g_ssim = (float(v) for v in got)
    assert abs(g_mse - mse) <= 1e-5 * mse, (g_mse, mse)
    assert abs(g_ssim - ssim) <= 2e-6, (g_ssim, ssim)
    assert abs(g_psnr - 10.0 * math.log10(1.0 / g_mse)) <= 1e-5, (g_psnr, g_mse)
    assert abs(g_psnr - psnr) <= 1e-3


@pytest.mark.parametrize("w,h,c,u8,window", [
    (123, 82, 3, True, 11), (123, 82, 4, False, 3), (31, 9, 3, False, 5), (31, 9, 4, True, 15),
    (64, 64, 3, True, 7), (64, 64, 4, False, 9), (1, 1, 3, False, 11), (1, 1, 4, True, 13),
    (400, 400, 3, True, 11), (400, 400, 4, False, 13), (1920, 1080, 3, True, 11), (1920, 1080, 4, False, 11)])
def test_metrics_match_float64_checker(dev, w, h, c, u8, window):
    import torch

    from brush_amd import eval_metrics

    pred, gt = _inputs(w, h, c, u8, seed=w * 7 + h + c + window)
    out = eval_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), window)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.device.type == "cuda"
    _check(out.cpu().numpy(), pred, gt, window)


def test_edge_semantics(dev):
    import ctypes as C

    import torch

    from brush_amd import _lib, eval_metrics

    w, h = 123, 82
    pred, gt = _inputs(w, h, 4, True, seed=5)
    tp = torch.from_numpy(pred).to(dev)
    # identical RGB: mse 0, psnr +inf, ssim 1
    same = eval_metrics(tp, tp[..., :3].contiguous()).cpu().numpy()
    assert same[0] == 0.0 and same[1] == np.inf and abs(float(same[2]) - 1.0) <= 1e-6, same
    # alpha of pred and of a 4-channel gt is never read
    base = eval_metrics(tp, torch.from_numpy(gt).to(dev)).cpu().numpy()
    pred2, gt2 = pred.copy(), gt.copy()
    pred2[..., 3] = np.random.default_rng(1).random((h, w))
    gt2[..., 3] = 255 - gt2[..., 3]
    alt = eval_metrics(torch.from_numpy(pred2).to(dev), torch.from_numpy(gt2).to(dev)).cpu().numpy()
    assert alt.tobytes() == base.tobytes()
    # u8 and the same image divided on the host give the same bits
    host = eval_metrics(tp, torch.from_numpy(_gt_f32(gt)).to(dev)).cpu().numpy()
    assert host.tobytes() == base.tobytes()
    # argument checks of the ABI
    l = _lib.lib()
    nb = C.c_size_t()
    _lib.check(l.brush_eval_workspace_size(w, h, C.byref(nb)), "ws")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    out = torch.empty(3, device=dev)
    tg = torch.from_numpy(gt).to(dev)
    s = torch.cuda.current_stream().cuda_stream

    def call(pred_p=tp.data_ptr(), gt_p=tg.data_ptr(), dt=_lib.EVAL_GT_U8, c=4, win=11, out_p=out.data_ptr(),
             ws_p=ws.data_ptr(), n=nb.value):
        return l.brush_eval_metrics(pred_p, gt_p, dt, w, h, c, win, out_p, ws_p, n, s)

    assert call() == 0
    for bad in (dict(win=1), dict(win=4), dict(win=17), dict(c=2), dict(c=1), dict(dt=7), dict(pred_p=None),
                dict(gt_p=None), dict(out_p=None), dict(ws_p=None)):
        assert call(**bad) == -1, bad
    assert call(n=nb.value - 8) == -2
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eval_metrics(tp, tg, window=12)
    with pytest.raises(ValueError):
        eval_metrics(tp, tg.to(torch.int32))
    with pytest.raises(ValueError):
        eval_metrics(tp[..., :3].contiguous(), tg)
    with pytest.raises(ValueError):
        eval_metrics(tp, tg[:-1])


def test_deterministic_and_graph_capturable(dev):
    import torch

    from brush_amd import eval_metrics

    pred, gt = _inputs(1920, 1080, 3, True, seed=9)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    first = eval_metrics(tp, tg).cpu().numpy().tobytes()
    for _ in range(10):
        assert eval_metrics(tp, tg).cpu().numpy().tobytes() == first
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = torch.full((3,), -1.0, device=dev)
    with torch.cuda.stream(s):
        eval_metrics(tp, tg, out=out)  # warm-up on the capture stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        eval_metrics(tp, tg, out=out)
    out.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == first


# ---------------------------------------------------------------------------- end to end: file -> cameras -> pixels
def _cloud(n, seed):
    """Seeded cloud around the origin (the test scenes look at it from radius ~4): SH degree 3, non-unit rotations."""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    log_scales = np.log(rng.uniform(0.004, 0.03, (n, 3))).astype(np.float32)
    quats = (rng.normal(size=(n, 4)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    sh = rng.uniform(-0.4, 0.4, (n, 16, 3)).astype(np.float32)
    sh[:, 0] = rng.uniform(-1.2, 1.2, (n, 3))
    raw_opac = rng.uniform(-2.0, 3.0, n).astype(np.float32)
    return means, sh, quats, raw_opac, log_scales


def _decode_ply(buf: bytes):
    """Inria-layout binary little-endian PLY decoded with numpy alone (not brush_amd.ply)."""
    end = buf.index(b"end_header\n") + len(b"end_header\n")
    head = buf[:end].decode("ascii").splitlines()
    assert "format binary_little_endian 1.0" in head
    names = [ln.split()[2] for ln in head if ln.startswith("property float ")]
    n = int([ln for ln in head if ln.startswith("element vertex")][0].split()[2])
    rec = np.frombuffer(buf, dtype=np.dtype([(nm, "<f4") for nm in names]), count=n, offset=end)
    col = lambda *ks: np.stack([rec[k] for k in ks], 1).astype(np.float32)
    rest = [k for k in names if k.startswith("f_rest_")]
    ncoef = len(rest) // 3 + 1
    sh = np.empty((n, ncoef, 3), np.float32)
    sh[:, 0] = col("f_dc_0", "f_dc_1", "f_dc_2")
    for ch in range(3):  # f_rest_* is channel-major: channel ch, coefficient k at ch * (ncoef - 1) + k - 1
        for k in range(1, ncoef):
            sh[:, k, ch] = rec[f"f_rest_{ch * (ncoef - 1) + k - 1}"]
    q = col("rot_0", "rot_1", "rot_2", "rot_3")
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    return dict(means=col("x", "y", "z"), log_scales=col("scale_0", "scale_1", "scale_2"), quats=q, sh=sh,
                raw_opac=rec["opacity"].astype(np.float32))


def _check_e2e(stats, expected_views, cloud):
    """expected_views: [(name suffix, hand-built uniforms, u8 image)] in scene order."""
    from brush_amd.render import uniforms_to_numpy
    from oracle import oracle as O

    assert len(stats.samples) == len(expected_views)
    for s, (suffix, u, img) in zip(stats.samples, expected_views):
        assert s.view.name.endswith(suffix), (s.view.name, suffix)
        h, w = img.shape[:2]
        assert tuple(s.rendered.shape) == (h, w, 3)
        E.uniforms_close(uniforms_to_numpy(s.aux), u)
        o_img, _ = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                        cloud["raw_opac"])
        mse, psnr, ssim = ref_metrics(o_img[..., :3], img[..., :3].astype(np.float32) / np.float32(255.0), 11)
        assert abs(s.psnr - psnr) <= 1e-3, (s.view.name, s.psnr, psnr)
        assert abs(s.ssim - ssim) <= 1e-5, (s.view.name, s.ssim, ssim)


def test_ply_on_nerf_synthetic_end_to_end(dev, tmp_path):
    """c1 plumbing: Splats.to_ply -> file -> Splats.from_ply, a NeRF-synthetic tree -> read_nerf_synthetic -> eval
    views -> eval_stats, against cameras built by hand from the JSON, the oracle's render and the float64 checker."""
    import torch

    import brush_amd
    from brush_amd import dataset as D

    src = brush_amd.Splats(*(torch.from_numpy(a).to(dev) for a in _cloud(104858, seed=11)))
    ply = tmp_path / "cloud.ply"
    ply.write_bytes(src.to_ply())
    rec = E.write_nerf(str(tmp_path / "nerf"), 400, 400, n_train=2, n_val=3)
    data = D.read_nerf_synthetic(str(tmp_path / "nerf"))
    splats = brush_amd.Splats.from_ply(str(ply), dev)
    stats = brush_amd.eval_stats(splats, data.eval, keep_aux=True)
    cloud = _decode_ply(ply.read_bytes())
    assert cloud["means"].shape == (104858, 3) and cloud["sh"].shape == (104858, 16, 3)
    expected = [(rel[2:] + ".png", E.nerf_uniforms(c2w, rec["camera_angle_x"], 400, 400, 3), img)
                for rel, c2w, img in rec["val"]]
    _check_e2e(stats, expected, cloud)
    assert all(s.aux is None for s in brush_amd.eval_stats(splats, data.eval, num_frames=2,
                                                           rng=np.random.default_rng(0)).samples)


def test_colmap_end_to_end_and_cli(dev, tmp_path):
    import torch

    import brush_amd
    from brush_amd import dataset as D

    src = brush_amd.Splats(*(torch.from_numpy(a).to(dev) for a in _cloud(30000, seed=12)))
    ply = tmp_path / "cloud.ply"
    ply.write_bytes(src.to_ply())
    rec = E.write_colmap(str(tmp_path / "colmap"), 320, 240, n_images=3)
    data = D.read_colmap(str(tmp_path / "colmap"), eval_split_every=1)
    splats = brush_amd.Splats.from_ply(str(ply), dev)
    stats = brush_amd.eval_stats(splats, data.eval, keep_aux=True)
    expected = [("images/" + nm, E.colmap_uniforms(q, t, rec["camera"], 3), img) for nm, q, t, img in rec["images"]]
    _check_e2e(stats, expected, _decode_ply(ply.read_bytes()))
    # the command line on the same files, in a child process
    out = tmp_path / "out.json"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "brush_amd.eval", str(ply), str(tmp_path / "colmap"),
                        "--eval-split-every", "1", "--json", str(out)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(out.read_text())
    assert [v["name"] for v in res["views"]] == [s.view.name for s in stats.samples]
    for v, s in zip(res["views"], stats.samples):
        assert abs(v["psnr"] - s.psnr) <= 1e-5 and abs(v["ssim"] - s.ssim) <= 1e-6
    assert abs(res["mean_psnr"] - stats.mean_psnr()) <= 1e-5 and abs(res["mean_ssim"] - stats.mean_ssim()) <= 1e-6
    assert len(r.stdout.strip().splitlines()) == 4 and "mean" in r.stdout.strip().splitlines()[-1]


def test_eval_does_not_disturb_training(dev):
    """Run A: six deterministic trainer steps with eval_stats after steps 2 and 4; run B: trainer.sync at the same two
    points instead.  Eval may flush the deferred SH steps (any render does) but must change nothing else."""
    import torch

    import brush_amd
    from brush_amd import dataset as D
    from brush_amd import render as R

    n, w, h = 4000, 160, 96
    cloud = H.synthetic_cloud(n, 3, seed=21, mean_mult=0.0003)
    cloud["log_scales"] = cloud["log_scales"] - 3.5
    cams = []
    for i in range(5):
        a = 2.0 * math.pi * i / 5
        cams.append(brush_amd.Camera([4.0 * math.sin(a), 0.0, -4.0 * math.cos(a)],
                                     [0.0, -math.sin(a / 2.0), 0.0, math.cos(a / 2.0)], 0.4, 0.3, (0.5, 0.5)))
    rng = np.random.default_rng(8)
    imgs = [(rng.random((h, w, 3)) * 255).astype(np.uint8) for _ in cams]
    gts = [torch.from_numpy(im.astype(np.float32) / np.float32(255.0)).to(dev) for im in imgs]
    scene = D.Scene([D.SceneView(f"v{i}", c, im) for i, (c, im) in enumerate(zip(cams, imgs))])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda: brush_amd.Splats(t(cloud["means"]), t(cloud["sh"]), t(cloud["quats"]), t(cloud["raw_opac"]),
                                  t(cloud["log_scales"]))
    cfg = lambda: brush_amd.TrainConfig(warmup_steps=0, max_refine_step=0, deferred_sh_adam=True)
    a, b = mk(), mk()
    ta, tb = brush_amd.SplatTrainer(a, cfg()), brush_amd.SplatTrainer(b, cfg())
    saved, R.DETERMINISTIC = R.DETERMINISTIC, True
    try:
        pending = 0
        for i in range(6):
            ta.step(a, cams[i % 5], gts[i % 5])
            tb.step(b, cams[i % 5], gts[i % 5])
            if i in (1, 3):
                pending += int(ta._lazy_pending and bool((ta._lazy_bufs[0] < ta.opt_time).any()))
                stats = brush_amd.eval_stats(a, scene)
                assert len(stats.samples) == 5 and all(math.isfinite(s.psnr) for s in stats.samples)
                tb.sync(b)
        assert pending > 0, "nothing was deferred before an eval: the test would prove nothing"
        ta.sync(a), tb.sync(b)
        for name in ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs"):
            assert torch.equal(getattr(a, name).detach(), getattr(b, name).detach()), name
        assert torch.equal(ta.moment1, tb.moment1) and torch.equal(ta.moment2, tb.moment2)
        assert torch.equal(ta._lazy_bufs[0], tb._lazy_bufs[0])
        assert ta.opt_time == tb.opt_time and ta.iter == tb.iter
    finally:
        R.DETERMINISTIC = saved


def test_not_slower_than_the_training_loss(dev):
    """At 1920x1080 one eval_metrics call takes no longer than one l1_ssim_loss call (ssim_weight 0.2: the SSIM
    forward with its derivative maps plus the backward), median of 20 event-timed calls each, 10 % allowance."""
    import torch

    from brush_amd import eval_metrics
    from brush_amd.train import l1_ssim_loss

    pred, gt = _inputs(1920, 1080, 3, False, seed=3)
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    tg8 = (tg * 255.0).round().to(torch.uint8)

    def median_ms(fn):
        fn(), fn()
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    out = torch.empty(3, device=dev)
    t_eval = median_ms(lambda: eval_metrics(tp, tg8, 11, out=out))
    t_eval_f32 = median_ms(lambda: eval_metrics(tp, tg, 11, out=out))
    t_loss = median_ms(lambda: l1_ssim_loss(tp, tg, 0.2, 11))
    print(f"1080p: eval_metrics u8 {t_eval * 1e3:.1f} us, f32 {t_eval_f32 * 1e3:.1f} us; "
          f"l1_ssim_loss {t_loss * 1e3:.1f} us")
    assert t_eval <= 1.1 * t_loss and t_eval_f32 <= 1.1 * t_loss
