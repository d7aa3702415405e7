"""GPU checks of the end-to-end training loop (brush_amd.train_loop): the loss on a u8 target
(brush_l1_ssim_loss_gt) against its f32 twin bit for bit, the trainer's trajectory on u8 against f32 targets, a
NeRF-synthetic scene trained from random splats, reproducibility, and no host synchronisation per step."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from brush_amd import render as R

    old = R.DETERMINISTIC
    R.DETERMINISTIC = True
    yield
    R.DETERMINISTIC = old


def _twins(w, h, channels, seed, dev):
    """(pred [h,w,4] f32, gt u8, gt f32 = u8 / 255 divided on the host) on the device."""
    import torch

    rng = np.random.default_rng(seed)
    pred = torch.from_numpy(rng.random((h, w, 4), dtype=np.float32)).to(dev)
    gt_np = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    gt_np[:3, :5] = 0  # exact matches: sign(0) and the clamp edges
    gt32 = torch.from_numpy(gt_np.astype(np.float32) / 255).to(dev)
    return pred, torch.from_numpy(gt_np).to(dev), gt32


def _bits(t):
    return t.detach().contiguous().view(-1).view(dtype=__import__("torch").int32).cpu().numpy()


# ---------------------------------------------------------------------------- 1. the loss on a u8 target
@pytest.mark.parametrize("w,h", [(67, 45), (200, 131), (1920, 1080)])
@pytest.mark.parametrize("channels", [3, 4])
def test_u8_loss_matches_f32_bitwise(dev, w, h, channels):
    from brush_amd.train import l1_ssim_loss

    pred, gt8, gt32 = _twins(w, h, channels, 1000 * w + channels, dev)
    cases = [(0.0, 11, s) for s in (1.0, 0.25)] + [(0.2, win, s) for win in (3, 11, 15) for s in (1.0, 0.25)]
    for ssim_w, win, scale in cases:
        l8, v8 = l1_ssim_loss(pred, gt8, ssim_w, win, scale)
        l32, v32 = l1_ssim_loss(pred, gt32, ssim_w, win, scale)
        what = f"{w}x{h}x{channels} ssim_weight={ssim_w} window={win} grad_scale={scale}"
        assert np.array_equal(_bits(l8), _bits(l32)), what
        assert np.array_equal(_bits(v8), _bits(v32)), what
        assert math.isfinite(float(l8.item())) and float(v8.abs().max()) > 0.0, what


def test_u8_loss_out_argument_and_bad_dtype(dev):
    import torch

    from brush_amd import _lib
    from brush_amd.train import l1_ssim_loss

    pred, gt8, gt32 = _twins(67, 45, 4, 7, dev)
    log = torch.full((5,), float("nan"), dtype=torch.float32, device=dev)
    ret, _ = l1_ssim_loss(pred, gt8, 0.2, 11, 1.0, out=log[2:3])
    ref, _ = l1_ssim_loss(pred, gt32, 0.2, 11, 1.0)
    host = log.cpu().numpy()
    assert ret.data_ptr() == log[2:3].data_ptr()
    assert np.isnan(host[[0, 1, 3, 4]]).all()
    assert host[2].view(np.int32) == ref.cpu().numpy()[0].view(np.int32)
    with pytest.raises(ValueError):
        l1_ssim_loss(pred, gt8, 0.2, 11, 1.0, out=log[1:3])
    with pytest.raises(ValueError):
        l1_ssim_loss(pred, gt8, 0.2, 11, 1.0, out=torch.empty(1, dtype=torch.float64, device=dev))

    l = _lib.lib()
    nbytes = C.c_size_t()
    _lib.check(l.brush_loss_workspace_size(67, 45, C.byref(nbytes)), "brush_loss_workspace_size")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    loss, v = torch.empty(1, device=dev), torch.empty_like(pred)
    stream = torch.cuda.current_stream().cuda_stream
    args = lambda dtype, nb=nbytes.value: (pred.data_ptr(), gt8.data_ptr(), dtype, 67, 45, 4, 0.2, 11, 1.0,
                                           loss.data_ptr(), v.data_ptr(), ws.data_ptr(), nb, stream)
    assert l.brush_l1_ssim_loss_gt(*args(2)) == -1  # BRUSH_ERR_INVALID_ARG
    assert l.brush_l1_ssim_loss_gt(*args(0xFFFFFFFF)) == -1
    assert l.brush_l1_ssim_loss_gt(*args(_lib.EVAL_GT_U8, 16)) == l.brush_l1_ssim_loss(
        pred.data_ptr(), gt32.data_ptr(), 67, 45, 4, 0.2, 11, 1.0, loss.data_ptr(), v.data_ptr(), ws.data_ptr(), 16,
        stream)  # the same status for a small workspace
    assert l.brush_l1_ssim_loss_gt(*args(_lib.EVAL_GT_U8)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 2. trainer trajectory, u8 against f32
def _ring_cameras(n, w, h, radius=4.0, height=1.0, offset=0.3):
    from brush_amd.dataset import nerf_camera

    cams = []
    for i in range(n):
        a = 2.0 * math.pi * i / n + offset
        c2w = E.look_at_gl((radius * math.cos(a), radius * math.sin(a), height)).astype(np.float32).astype(np.float64)
        cams.append((c2w, nerf_camera(c2w, 0.6911112070083618, w, h)))
    return cams


@pytest.mark.parametrize("deferred", [True, False])
def test_trainer_trajectory_u8_equals_f32(dev, deterministic, deferred):
    import torch

    from brush_amd import Splats, SplatTrainer, TrainConfig

    w, h = 96, 80
    cams = _ring_cameras(4, w, h)
    imgs = [E.noise_image(w, h, 3 + (i % 2), 50 + i) for i in range(4)]
    gt8 = [torch.from_numpy(im).to(dev) for im in imgs]
    gt32 = [torch.from_numpy(im.astype(np.float32) / 255).to(dev) for im in imgs]
    cfg = TrainConfig(warmup_steps=5, refine_every=10, deferred_sh_adam=deferred, densify_grad_thresh=1e-5)
    results, refines = [], []
    for gts in (gt8, gt32):
        splats = Splats.from_random_config(1024, 3, (np.full(3, -1.0), np.full(3, 1.0)), np.random.default_rng(3), dev)
        tr = SplatTrainer(splats, cfg)
        nref = 0
        for i in range(40):
            tr.step(splats, cams[i % 4][1], gts[i % 4], 1.0)
            nref += tr.last_refine is not None
        tr.sync(splats)
        refines.append(nref)
        results.append({k: _bits(getattr(splats, k)) for k in ("means", "log_scales", "rotation", "raw_opacity",
                                                                 "sh_coeffs")})
    assert refines[0] >= 2 and refines[0] == refines[1]
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), k


# ---------------------------------------------------------------------------- 3. end to end
def _write_scene(root, dev, w=128, h=128, n_train=16, n_val=4):
    """A NeRF-synthetic tree of renders of a known cloud (3000 splats in a box around the origin)."""
    import torch

    from brush_amd import Splats

    rng = np.random.default_rng(11)
    known = Splats.from_random_config(3000, 0, (np.full(3, -0.8), np.full(3, 0.8)), rng, dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.06))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    fovx = 0.6911112070083618
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i, (c2w, cam) in enumerate(_ring_cameras(n, w, h, 4.0, 1.0, off)):
            with torch.no_grad():
                pred, _ = known.render(cam, (w, h), False)
            img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(E.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    return _write_scene(str(tmp_path_factory.mktemp("train_loop_scene")), dev)


def _cfg():
    from brush_amd import TrainConfig

    return TrainConfig(warmup_steps=50, refine_every=50)


def test_train_scene_end_to_end(dev, scene_dir, tmp_path):
    import torch

    from brush_amd import Splats
    from brush_amd.eval import eval_stats
    from brush_amd.train_loop import load_dataset, train_scene

    data, points = load_dataset(scene_dir)
    assert points is None and len(data.train.views) == 16 and len(data.eval.views) == 4
    rows = []
    splats, log = train_scene(data, _cfg(), steps=600, init_count=2000, sh_degree=3, seed=5, eval_every=200,
                              on_eval=lambda r, s: rows.append(r))
    assert [r.step for r in rows] == [0, 200, 400, 600] and log.evals == rows
    print("train_loop e2e psnr by step:", [(r.step, round(r.psnr, 3), r.splats) for r in rows])
    # measured on the MI355X in two runs: 12.99 dB at step 0 -> 26.17 / 26.61 dB at step 600 (+13.2 / +13.6 dB;
    # 2000 -> ~25 800 splats); the threshold asks for under half of that gain
    assert rows[-1].psnr > rows[0].psnr + 6.0
    assert rows[-1].splats != 2000  # refinement ran
    assert log.losses.shape == (600,) and np.isfinite(log.losses).all()
    assert float(np.mean(log.losses[-50:])) < float(np.mean(log.losses[:50]))
    assert log.image_bytes == 16 * 128 * 128 * 3

    # the returned splats are current: exported, read back (from_ply normalises rotations) and evaluated, they give
    # the bits of the same splats with normalised rotations
    ply = splats.to_ply()
    back = Splats.from_ply(ply, dev)
    for k in ("means", "log_scales", "raw_opacity", "sh_coeffs"):
        assert np.array_equal(_bits(getattr(back, k)), _bits(getattr(splats, k))), k
    twin = Splats(splats.means, splats.sh_coeffs, splats.rotation, splats.raw_opacity, splats.log_scales)
    twin.norm_rotations()
    a = eval_stats(back, data.eval)
    b = eval_stats(twin, data.eval)
    for x, y in zip(a.samples, b.samples):
        assert np.float32(x.psnr).view(np.int32) == np.float32(y.psnr).view(np.int32)
        assert np.float32(x.ssim).view(np.int32) == np.float32(y.ssim).view(np.int32)
    assert abs(eval_stats(splats, data.eval).mean_psnr() - a.mean_psnr()) < 1e-3
    torch.cuda.synchronize()


def test_train_loop_cli(scene_dir, tmp_path):
    out_ply, out_json = str(tmp_path / "out.ply"), str(tmp_path / "log.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "60", "--eval-every", "30",
                        "--eval-views", "2", "--init-count", "1000", "--export", out_ply, "--json", out_json],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert [ln.split("\t")[0] for ln in lines[:3]] == ["step 0", "step 30", "step 60"] and lines[-1].startswith("done:")
    assert os.path.getsize(out_ply) > 1000
    with open(out_json) as f:
        log = json.load(f)
    assert len(log["losses"]) == 60 and [e["step"] for e in log["evals"]] == [0, 30, 60]


# ---------------------------------------------------------------------------- 4. reproducible
def test_train_scene_reproducible(dev, scene_dir, deterministic):
    from brush_amd.train_loop import load_dataset, train_scene

    data, _ = load_dataset(scene_dir)
    plys = []
    for _ in range(2):
        splats, log = train_scene(data, _cfg(), steps=120, init_count=1000, sh_degree=3, seed=9)
        plys.append(splats.to_ply())
    assert plys[0] == plys[1]


# ---------------------------------------------------------------------------- 5. no host sync per step
def test_loop_steps_do_not_synchronise(dev, scene_dir):
    import torch

    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop, load_dataset

    data, _ = load_dataset(scene_dir)
    loop = TrainLoop(data, TrainConfig(warmup_steps=5, refine_every=50), steps=30, init_count=1000, seed=1)
    loop.step()  # the first step fills the deferred-SH table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # the mode sees a readback on this torch build
            loop.losses[0].item()
        with pytest.raises(RuntimeError):  # and an upload from pageable host memory, as image_to_tensor's
            torch.from_numpy(loop.dataset.train.views[0].image.copy()).to(dev)
        for _ in range(20):  # optimizer steps 2..21: past the warmup, before the first refinement (step 51)
            loop.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loop.trainer.last_refine is None and loop.done == 21
    _, log = loop.finish()
    assert np.isfinite(log.losses[:21]).all() and (log.losses[21:] == 0).all()
