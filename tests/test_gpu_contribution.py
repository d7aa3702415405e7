"""GPU checks of pruning by rendered contribution (brush_render_contributions, brush_amd/contribution.py):
the hand-made kernel inputs of tests/contrib_cases.py against the float64 reference of tests/contrib_ref64.py (counts
exactly, max and sum inside the allowance, wrong references rejected, exact cases by bits), the replay's fidelity to
real forwards, the invariance of the views under the exact pruning rule, accumulation and repeatability, and the
training loop's pruning step with both command lines."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import contrib_ref64 as R
from tests import helpers as H
from tests import margins

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CC.all_cases()


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from brush_amd import render as Rn

    old = Rn.DETERMINISTIC
    Rn.DETERMINISTIC = True
    yield
    Rn.DETERMINISTIC = old


def _bits(t):
    import torch

    return t.detach().contiguous().view(-1).view(dtype=torch.int32).cpu().numpy()


# ---------------------------------------------------------------------------- 1. hand-made kernel inputs
def _run_case(case, dev, repeat=1):
    """The kernel on a hand-made case through contributions_from_aux; the aux arrays the entry does not read are
    one-word dummies.  Returns the result as numpy arrays."""
    import torch

    from brush_amd import _lib
    from brush_amd.contribution import ContributionBuffers, contributions_from_aux
    from brush_amd.render import RenderAux

    def t(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)

    dummy = torch.zeros(1, dtype=torch.int32, device=dev)
    aux = RenderAux(projected_splats=t(case["projected"], torch.float32), uniforms_buffer=dummy,
                    num_intersections=dummy, num_visible=t([case["num_visible"]], torch.int32), final_index=dummy,
                    cum_tiles_hit=dummy, tile_bins=t(case["tile_bins"], torch.int32),
                    compact_gid_from_isect=t(case["isect"], torch.int32),
                    global_from_compact_gid=t(case["g_from_c"], torch.int32), compact_from_global_gid=dummy,
                    overflow=dummy, max_intersects=int(case["isect"].shape[0]))
    u = _lib.BrushUniforms()
    u.img_size[:] = [case["w"], case["h"]]
    u.tile_bounds[:] = [case["tile_bins"].shape[1], case["tile_bins"].shape[0]]
    bufs = ContributionBuffers(case["n"], dev)
    for _ in range(repeat):
        contributions_from_aux(u, aux, None, bufs, check=False)
    c, _ = bufs.read()
    return dict(max=c.max.numpy(), sum=c.sum.numpy(), hits=c.hits.numpy(), stops=c.stops.numpy())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_made_case(dev, case):
    ref = R.walk(case)
    got = _run_case(case, dev)
    g = R.gate(got, ref)
    print(f"{case['name']}: hits {int(ref['hits'].sum())} stops {int(ref['stops'].sum())} "
          f"max err/tol {g['ratio_max']:.4f} sum err/tol {g['ratio_sum']:.4f}")
    margins.record("contrib", "max", g["ratio_max"])
    margins.record("contrib", "sum", g["ratio_sum"])
    assert np.array_equal(got["hits"], ref["hits"]) and np.array_equal(got["stops"], ref["stops"])
    assert g["ratio_max"] <= 1.0 and g["ratio_sum"] <= 1.0, g
    margins.check_growth("contrib", "max", g["ratio_max"])
    margins.check_growth("contrib", "sum", g["ratio_sum"])
    # rows of ids outside the lists, and of splats the walk never reaches, stay zero
    for k in ("max", "sum", "hits", "stops"):
        assert not got[k][~ref["touched"]].any(), k
    # the wrong references fail the gate wherever they differ from the right one beyond its tolerance
    for m in R.MUTATIONS:
        wrong = R.walk(case, mutate=m)
        if not R.passes(R.gate(ref, wrong)):
            assert not R.passes(R.gate(got, wrong)), m


def test_each_wrong_reference_fails_on_the_device(dev):
    by_name = {c["name"]: c for c in CASES}
    for m, name in (("noclamp", "clamped"), ("stop_as_hit", "saturating"), ("ignore_T", "random_200"),
                    ("last_max", "random_200")):
        got = _run_case(by_name[name], dev)
        assert R.passes(R.gate(got, R.walk(by_name[name])))
        assert not R.passes(R.gate(got, R.walk(by_name[name], mutate=m))), (m, name)


def test_exact_cases_by_bits(dev):
    got = _run_case(CC.exact_single(), dev)
    ref = R.walk(CC.exact_single())
    assert got["max"].view(np.uint32)[0] == np.float32(CC.EXACT_O).view(np.uint32)
    assert int(got["hits"][0]) == int(ref["hits"][0]) > 0 and int(got["stops"][0]) == 0
    got = _run_case(CC.exact_pair(), dev)
    want = np.float32(0.25) * (np.float32(1.0) - np.float32(0.25))
    assert got["max"].view(np.uint32)[0] == np.float32(0.25).view(np.uint32)
    assert got["max"].view(np.uint32)[1] == np.float32(want).view(np.uint32)


def test_buffers_accumulate_across_calls(dev):
    """Two replays into the same buffers: counts and sums double exactly, the max stays."""
    case = CC.random_case()
    one, two = _run_case(case, dev), _run_case(case, dev, repeat=2)
    assert np.array_equal(two["hits"], 2 * one["hits"]) and np.array_equal(two["stops"], 2 * one["stops"])
    assert np.array_equal(two["sum"], 2 * one["sum"])
    assert np.array_equal(two["max"].view(np.uint32), one["max"].view(np.uint32))


# ---------------------------------------------------------------------------- 2. replay fidelity on real forwards
def _camera(w, h, position=None):
    import brush_amd

    c = H.reference_test_camera(w, h)
    return brush_amd.Camera(position or c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def _forward(splats, cam, size, antialiased=False, deterministic=None):
    import torch

    from brush_amd import render as Rn

    with torch.no_grad():
        rot = splats.rotation.detach()
        norm_rot = (rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))).contiguous()
        return Rn._forward_impl(cam, size, splats.means.detach(), splats.log_scales.detach(), norm_rot,
                                splats.sh_coeffs.detach(), splats.raw_opacity.detach(), False, None,
                                deterministic=deterministic, expect_backward=False, antialiased=antialiased)


def _replay(splats, cam, size, dev, img_override=None, **kw):
    from brush_amd.contribution import ContributionBuffers, contributions_from_aux

    img, aux, u = _forward(splats, cam, size, **kw)
    bufs = ContributionBuffers(splats.num_splats(), dev)
    contributions_from_aux(u, aux, img if img_override is None else img_override(img), bufs, check=True)
    c, bad = bufs.read()
    return c, bad, img, aux


@pytest.mark.parametrize("name,size,kw", [
    ("tiny_case", None, {}), ("basic_case", None, {}), ("basic_case", (77, 35), {}),
    ("basic_case", None, {"antialiased": True}), ("basic_case", None, {"deterministic": True}),
    ("basic_case", (50, 41), {"antialiased": True, "deterministic": True})])
def test_replay_reproduces_the_forward(dev, name, size, kw):
    import brush_amd

    d = H.load_case(name)
    h, w, _ = d["out_img"].shape
    w, h = size or (w, h)
    splats = brush_amd.Splats.from_safetensors(d, dev)
    c, bad, img, aux = _replay(splats, _camera(w, h), (w, h), dev, **kw)
    assert bad == 0
    assert int(c.hits.sum()) > 0 and float(c.max.max()) > 0.0
    # a splat that was added somewhere has a positive max and sum, and the other way round
    assert np.array_equal((c.hits > 0).numpy(), (c.max > 0).numpy())
    assert np.array_equal((c.hits > 0).numpy(), (c.sum > 0).numpy())
    # the summed weight over all splats is the summed alpha of the image (every added fac is a term of 1 - T up to
    # rounding: 1 - T = sum fac exactly in real arithmetic)
    total = float(img[..., 3].double().sum())
    assert abs(float(c.sum.sum()) - total) <= 1e-4 * max(total, 1.0)


def test_replay_with_no_visible_splat(dev):
    import torch

    import brush_amd

    d = H.load_case("basic_case")
    h, w, _ = d["out_img"].shape
    splats = brush_amd.Splats.from_safetensors(d, dev)
    with torch.no_grad():
        splats.means[:, 2] -= 100.0  # everything behind the camera
    c, bad, img, aux = _replay(splats, _camera(w, h), (w, h), dev)
    assert aux.read_num_visible() == 0 and bad == 0
    assert not c.hits.any() and not c.stops.any() and not c.max.any() and not c.sum.any()


def test_self_check_counts_one_flipped_alpha_bit(dev):
    import brush_amd

    d = H.load_case("basic_case")
    h, w, _ = d["out_img"].shape
    splats = brush_amd.Splats.from_safetensors(d, dev)

    def flip(img):
        import torch

        out = img.clone()
        word = out.view(torch.int32)
        word[h // 2, w // 2, 3] ^= 1
        return out

    _, bad, _, _ = _replay(splats, _camera(w, h), (w, h), dev, img_override=flip)
    assert bad == 1


# ---------------------------------------------------------------------------- 3. invariance under the exact rule
W3, H3 = 64, 48


def _wall_scene(dev):
    """Seeded: 150 small splats in front, three layers of an opaque wall, 30 splats behind the wall and 30 outside every
    frustum.  Returns (splats, index arrays of the hidden and the off-screen splats, the three cameras)."""
    import torch

    import brush_amd

    rng = np.random.default_rng(21)
    front = np.c_[rng.uniform(-2.5, 2.5, (150, 2)), rng.uniform(-1.0, 1.0, 150)]
    gx, gy = np.meshgrid(np.arange(-5.0, 5.01, 1.0), np.arange(-5.0, 5.01, 1.0))
    wall = np.concatenate([np.c_[gx.ravel(), gy.ravel(), np.full(gx.size, z)] for z in (3.0, 3.2, 3.4)])
    hidden = np.c_[rng.uniform(-1.5, 1.5, (30, 2)), rng.uniform(5.5, 6.5, 30)]
    off = np.c_[rng.uniform(40.0, 60.0, (30, 2)) * rng.choice([-1.0, 1.0], (30, 2)), rng.uniform(-1.0, 1.0, 30)]
    means = np.concatenate([front, wall, hidden, off]).astype(np.float32)
    n = means.shape[0]
    log_scales = np.full((n, 3), math.log(0.15), np.float32)
    log_scales[150:150 + wall.shape[0]] = math.log(0.8)
    raw_opac = rng.uniform(-1.0, 2.0, n).astype(np.float32)
    raw_opac[150:150 + wall.shape[0]] = 10.0
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.uniform(-0.5, 1.5, (n, 1, 3)).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=dev)
    splats = brush_amd.Splats(t(means), t(sh), t(quats), t(raw_opac), t(log_scales))
    i_hidden = np.arange(150 + wall.shape[0], 150 + wall.shape[0] + 30)
    i_off = np.arange(150 + wall.shape[0] + 30, n)
    cams = [brush_amd.Camera(p, [0.0, 0.0, 0.0, 1.0], 0.6, 0.6 * H3 / W3, (0.5, 0.5))
            for p in ([-1.0, 0.0, -8.0], [1.0, 0.2, -8.0], [0.0, -0.5, -7.0])]
    return splats, i_hidden, i_off, cams


def test_exact_rule_leaves_every_view_bitwise_identical(dev):
    import torch

    from brush_amd import prune_mask, splat_contributions

    splats, i_hidden, i_off, cams = _wall_scene(dev)
    views = [(cam, (W3, H3)) for cam in cams]
    c = splat_contributions(splats, views)  # check=True: raises on a replay that differs from its forward
    assert c.views == 3
    mask = prune_mask(c, min_max=0.0)
    assert mask[torch.as_tensor(i_hidden)].all() and mask[torch.as_tensor(i_off)].all()
    assert 60 <= int(mask.sum()) < splats.num_splats() - 100
    assert int(c.stops.sum()) > 0  # the wall saturates pixels: stoppers exist in this scene
    kept = splats.select((~mask).to(dev))
    assert kept.num_splats() == splats.num_splats() - int(mask.sum())
    with torch.no_grad():
        for cam in cams:
            a, _ = splats.render(cam, (W3, H3), False)
            b, _ = kept.render(cam, (W3, H3), False)
            assert np.array_equal(_bits(a), _bits(b))  # all four channels
    # the kept set is stable: measured again, nothing more falls under the exact rule
    assert not prune_mask(splat_contributions(kept, views), min_max=0.0).any()


def test_a_splat_that_only_stops_pixels_cannot_be_removed(dev):
    """Four flat splats (1000 units wide: about 1000 px, so their alpha varies by under 1e-4 over the frame) over a
    16 x 16 frame, front to back: A1 (opacity 1: alpha clamps to 0.999, T = 1e-3), A2 (0.85:
    T ~ 1.5e-4), S (0.5: would take T to ~7.5e-5 <= 1e-4, so it ends every pixel WITHOUT being added) and B (0.1).  S has
    hits == 0 and stops == 256; with S removed B is added (T 0.9 ~ 1.35e-4 > 1e-4) and the image changes.  That is why
    stops are counted, and why the exact rule keeps S."""
    import torch

    import brush_amd
    from brush_amd import prune_mask, splat_contributions

    logit = lambda p: math.log(p / (1.0 - p))
    means = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [0.0, 0.0, 3.0]], device=dev)
    raw = torch.tensor([20.0, logit(0.85), logit(0.5), logit(0.1)], device=dev)
    scales = torch.full((4, 3), math.log(1000.0), device=dev)
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 4, device=dev)
    sh = torch.tensor([[[0.5, 0.2, 0.1]], [[0.1, 0.9, 0.3]], [[1.0, 1.0, 1.0]], [[0.2, 0.4, 1.5]]], device=dev)
    splats = brush_amd.Splats(means, sh, quats, raw, scales)
    cam = _camera(16, 16)
    c = splat_contributions(splats, [(cam, (16, 16))])
    assert c.hits.tolist() == [256, 256, 0, 0] and c.stops.tolist() == [0, 0, 256, 0]
    assert float(c.max[2]) == 0.0 and float(c.sum[2]) == 0.0
    assert prune_mask(c, min_max=0.0).tolist() == [False, False, False, True]  # B is never reached; S stays
    with torch.no_grad():
        full, _ = splats.render(cam, (16, 16), False)
        without_b, _ = splats.select(torch.tensor([0, 1, 2])).render(cam, (16, 16), False)
        without_s, _ = splats.select(torch.tensor([0, 1, 3])).render(cam, (16, 16), False)
    assert np.array_equal(_bits(full), _bits(without_b))
    assert not np.array_equal(_bits(full), _bits(without_s))
    assert not np.array_equal(_bits(full[..., 3]), _bits(without_s[..., 3]))  # B's weight shows in alpha at every pixel


# ---------------------------------------------------------------------------- 4. accumulation and repeatability
def test_views_accumulate_and_runs_repeat_bitwise(dev):
    from brush_amd import splat_contributions

    splats, _, _, cams = _wall_scene(dev)
    a, b = (cams[0], (W3, H3)), (cams[1], (W3, H3))
    both = splat_contributions(splats, [a, b])
    parts = splat_contributions(splats, [a]).accumulate(splat_contributions(splats, [b]))
    again = splat_contributions(splats, [a, b])
    for other in (parts, again):
        assert both.views == other.views == 2
        assert np.array_equal(both.max.numpy().view(np.uint32), other.max.numpy().view(np.uint32))
        assert np.array_equal(both.sum.numpy().view(np.uint64), other.sum.numpy().view(np.uint64))
        assert np.array_equal(both.hits.numpy(), other.hits.numpy())
        assert np.array_equal(both.stops.numpy(), other.stops.numpy())
    down = splat_contributions(splats, [a], downscale=2)  # 32 x 24: about a quarter of the pixels
    one = splat_contributions(splats, [a])
    assert 0.15 * int(one.hits.sum()) < int(down.hits.sum()) < 0.4 * int(one.hits.sum())


# ---------------------------------------------------------------------------- 5. the training loop and the CLIs
def _write_scene(root, dev, w=64, h=64, n_train=6, n_val=2):
    """A small NeRF-synthetic tree of renders of a known cloud (the shape of tests/test_gpu_train_loop.py's scene)."""
    import torch

    from brush_amd import Splats
    from brush_amd.dataset import nerf_camera
    from tests import eval_data as E

    rng = np.random.default_rng(11)
    known = Splats.from_random_config(800, 0, (np.full(3, -0.8), np.full(3, 0.8)), rng, dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.08))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    fovx = 0.6911112070083618
    for split, n, off in (("train", n_train, 0.1), ("val", n_val, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(n):
            ang = 2.0 * math.pi * i / n + off
            c2w = E.look_at_gl((4.0 * math.cos(ang), 4.0 * math.sin(ang), 1.0)).astype(np.float32).astype(np.float64)
            with torch.no_grad():
                pred, _ = known.render(nerf_camera(c2w, fovx, w, h), (w, h), False)
            img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(E.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    return _write_scene(str(tmp_path_factory.mktemp("contribution_scene")), dev)


FAR = 100  # splats of the initial cloud that no training view can see


def _loop(data, prune_at, prune_min, steps=60):
    """A loop on 1500 random splats plus FAR copies of the first ones lifted 60 units above the scene, outside every
    frustum: they get no gradient, keep their initial opacity of 0.1 and survive the refinement's own pruning."""
    import torch

    from brush_amd import Splats, TrainConfig
    from brush_amd.train_loop import TrainLoop, random_init_bounds

    dev = torch.device("cuda:0")
    base = Splats.from_random_config(1500, 1, random_init_bounds(data.train), np.random.default_rng(4), dev)
    with torch.no_grad():
        cat = lambda t, shift=None: torch.cat([t, t[:FAR] if shift is None else t[:FAR] + shift])
        init = Splats(cat(base.means, torch.tensor([0.0, 0.0, 60.0], device=dev)), cat(base.sh_coeffs),
                      cat(base.rotation), cat(base.raw_opacity), cat(base.log_scales))
    cfg = TrainConfig(warmup_steps=10, refine_every=20, contribution_prune_at=prune_at,
                      contribution_prune_min=prune_min)
    return TrainLoop(data, cfg, steps=steps, init=init, sh_degree=1, seed=4)


def test_train_loop_prunes_at_the_listed_step(dev, scene_dir, deterministic):
    import torch

    from brush_amd.train_loop import load_dataset

    data, _ = load_dataset(scene_dir)
    loop = _loop(data, (40,), 0.01)
    counts = []
    for i in range(60):
        loop.step()
        counts.append(loop.splats.num_splats())
        if i == 40:
            # the optimizer state and the refinement statistics start over, as after a refinement
            tr = loop.trainer
            n = loop.splats.num_splats()
            assert tr.opt_time == 0 and not tr.moment1.any() and not tr.moment2.any()
            assert tr.moment1.numel() == n * (11 + 3 * 4) and tr.grad_2d_accum.shape == (n,)
            assert not tr.grad_2d_accum.any() and not tr.xy_grad_counts.any()
    splats, log = loop.finish()
    assert len(log.prunes) == 1
    step, before, after = log.prunes[0]
    print("prune at step", step, ":", before, "->", after)
    assert step == 40 and after <= before - FAR and counts[40] == after and counts[39] == before
    assert log.to_json()["prunes"] == [[40, before, after]]
    assert log.losses.shape == (60,) and np.isfinite(log.losses).all()  # the later steps ran
    assert splats.num_splats() == counts[-1]
    torch.cuda.synchronize()


def test_exact_prune_keeps_the_training_views_bitwise(dev, scene_dir, deterministic):
    import torch

    from brush_amd.train_loop import load_dataset

    data, _ = load_dataset(scene_dir)
    loop = _loop(data, (), 0.0, steps=45)
    for _ in range(41):
        loop.step()
    loop.trainer.sync(loop.splats)
    views = data.train.views

    def renders():
        with torch.no_grad():
            return [_bits(loop.splats.render(v.camera, (64, 64), False)[0]) for v in views]

    just_before = renders()
    loop.config.contribution_prune_min = 0.0
    before, after = loop.prune_by_contribution()
    print("exact prune:", before, "->", after)
    assert after <= before - FAR and loop.log.prunes == [(41, before, after)]  # at least the unseen splats go
    for a, b in zip(just_before, renders()):
        assert np.array_equal(a, b)
    for _ in range(4):  # and the loop goes on
        loop.step()
    assert np.isfinite(loop.finish()[1].losses).all()


def test_idle_option_leaves_the_trajectory_bitwise(dev, scene_dir, deterministic):
    """() and a schedule that never comes due give the same run bit for bit, and a run with a prune at step 40 is that
    same run up to and including step 40's loss."""
    from brush_amd.train_loop import load_dataset

    data, _ = load_dataset(scene_dir)
    runs = {}
    for key, at in (("none", ()), ("idle", (1000,)), ("prune", (40,))):
        loop = _loop(data, at, 0.01, steps=50)
        for _ in range(50):
            loop.step()
        splats, log = loop.finish()
        runs[key] = (splats.to_ply(), log.losses.view(np.uint32), log.prunes)
    assert runs["none"][0] == runs["idle"][0] and np.array_equal(runs["none"][1], runs["idle"][1])
    assert runs["none"][2] == [] and runs["idle"][2] == []
    assert np.array_equal(runs["none"][1][:41], runs["prune"][1][:41]) and len(runs["prune"][2]) == 1


def test_command_lines_round_trip(scene_dir, tmp_path):
    """train_loop with a prune, then brush_amd.prune on its export: a PLY of the kept count and a JSON."""
    from brush_amd.ply import load_splat_from_ply

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    trained, log_json = str(tmp_path / "trained.ply"), str(tmp_path / "log.json")
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "50", "--init-count", "1500",
                        "--sh-degree", "1", "--contribution-prune-at", "30", "--contribution-prune-min", "0.01",
                        "--export", trained, "--json", log_json], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(log_json) as f:
        log = json.load(f)
    assert len(log["prunes"]) == 1 and log["prunes"][0][0] == 30 and log["prunes"][0][2] <= log["prunes"][0][1]
    out_ply, out_json = str(tmp_path / "pruned.ply"), str(tmp_path / "pruned.json")
    r = subprocess.run([sys.executable, "-m", "brush_amd.prune", trained, scene_dir, "--keep-fraction", "0.5", "--by", "sum",
                        "--views", "all", "--export", out_ply, "--json", out_json], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("splats\tbefore ") and lines[1].startswith("eval (2 views)\tpsnr ")
    with open(out_json) as f:
        res = json.load(f)
    n0 = load_splat_from_ply(trained)["means"].shape[0]
    assert res["splats_before"] == n0 == log["num_splats"] and res["splats_after"] == math.ceil(0.5 * n0)
    assert load_splat_from_ply(out_ply)["means"].shape[0] == res["splats_after"]
    assert res["num_views"] == 8 and sum(res["max_histogram"].values()) == n0
    assert np.isfinite(res["eval_before"]["psnr"]) and np.isfinite(res["eval_after"]["psnr"])
