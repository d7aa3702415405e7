"""GPU checks of error-driven densification in the trainer and the training loop (TrainConfig.densify_by = "error",
SplatTrainer.set_densify_scores / will_refine, TrainLoop.score_errors, revised_opacity) on a tiny scene written on the
fly: the score passes run in front of exactly the refining steps, the growth and count caps hold, runs repeat bitwise,
the default configuration is the run without the options, a refinement without scores is refused, the revised opacity
touches only the documented rows, and the command line writes the new fields."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 40
N_INIT = 600
REFINING = (5, 9)  # warmup_steps=2, refine_every=4, 12 steps: iter >= 2 and iter % 4 == 1


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


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory, dev):
    """A small NeRF-synthetic tree of renders of a known cloud: 5 training views and 1 eval view of 48 x 40."""
    import torch

    from brush_amd import Splats
    from brush_amd.dataset import nerf_camera
    from tests import eval_data as E

    root = str(tmp_path_factory.mktemp("error_densify_scene"))
    rng = np.random.default_rng(13)
    known = Splats.from_random_config(400, 0, (np.full(3, -0.8), np.full(3, 0.8)), rng, dev)
    with torch.no_grad():
        known.log_scales.fill_(math.log(0.1))
        known.raw_opacity.fill_(math.log(0.8 / 0.2))
    fovx = 0.6911112070083618
    for split, n, off in (("train", 5, 0.1), ("val", 1, 0.5)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(n):
            ang = 2.0 * math.pi * i / n + off
            c2w = E.look_at_gl((4.0 * math.cos(ang), 4.0 * math.sin(ang), 1.0)).astype(np.float32).astype(np.float64)
            with torch.no_grad():
                pred, _ = known.render(nerf_camera(c2w, fovx, W, H), (W, H), False)
            img = np.clip(np.round(pred[..., :3].cpu().numpy() * 255.0), 0, 255).astype(np.uint8)
            with open(os.path.join(root, split, f"r_{i}.png"), "wb") as f:
                f.write(E.png_bytes(img))
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.0, "transform_matrix": c2w.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": fovx, "frames": frames}, f)
    return root


@pytest.fixture(scope="module")
def data(scene_dir):
    from brush_amd.train_loop import load_dataset

    return load_dataset(scene_dir)[0]


def _loop(data, steps=12, **cfg):
    import torch

    from brush_amd import Splats, TrainConfig
    from brush_amd.train_loop import TrainLoop, random_init_bounds

    dev = torch.device("cuda:0")
    init = Splats.from_random_config(N_INIT, 1, random_init_bounds(data.train), np.random.default_rng(4), dev)
    return TrainLoop(data, TrainConfig(warmup_steps=2, refine_every=4, **cfg), steps=steps, init=init, sh_degree=1,
                     seed=4)


def _run(data, steps=12, **cfg):
    """(ply bytes, loss bits, counts after every step, refinement stats by step, log) of one run."""
    loop = _loop(data, steps, **cfg)
    counts, refines = [], {}
    for i in range(steps):
        before = loop.splats.num_splats()
        loop.step()
        counts.append(loop.splats.num_splats())
        if loop.trainer.last_refine is not None:
            refines[i] = (before, loop.trainer.last_refine)
    splats, log = loop.finish()
    return splats.to_ply(), log.losses.view(np.uint32).copy(), counts, refines, log


ERR = dict(densify_by="error", densify_error_thresh=0.02, densify_error_views=3, densify_growth=0.1)


def test_error_passes_caps_and_repeatability(dev, data, deterministic):
    ply, losses, counts, refines, log = _run(data, **ERR)
    assert log.densify_by == "error" and log.error_passes == [(s, 3) for s in REFINING]
    assert sorted(refines) == list(REFINING)
    assert log.to_json()["error_passes"] == [[s, 3] for s in REFINING] and log.to_json()["densify_by"] == "error"
    grown = 0
    for s in REFINING:
        before, st = refines[s]
        cap = math.ceil(0.1 * before)
        print(f"step {s}: {before} -> {counts[s]} (split {st.num_split}, cloned {st.num_cloned}, cap {cap})")
        assert st.num_split + st.num_cloned <= cap
        assert counts[s] - before <= cap
        grown += st.num_split + st.num_cloned
    assert grown > 0  # the rule densified something on this scene
    assert np.isfinite(log.losses).all()
    ply2, losses2, counts2, _, _ = _run(data, **ERR)
    assert ply == ply2 and np.array_equal(losses, losses2) and counts == counts2
    # every training view: 0 means all five
    _, _, _, _, log_all = _run(data, steps=6, **dict(ERR, densify_error_views=0))
    assert log_all.error_passes == [(5, 5)]


def test_max_splats_holds(dev, data, deterministic):
    limit = N_INIT + 7
    _, _, counts, refines, _ = _run(data, **dict(ERR, densify_max_splats=limit))
    assert max(counts) <= limit and sorted(refines) == list(REFINING)
    before, st = refines[REFINING[0]]
    assert 0 < st.num_split + st.num_cloned <= limit - before
    _, _, counts, refines, _ = _run(data, steps=6, **dict(ERR, densify_max_splats=N_INIT - 100))  # below the count
    assert refines[5][1].num_split + refines[5][1].num_cloned == 0 and max(counts) <= N_INIT


def test_default_fields_are_the_run_without_them(dev, data, deterministic):
    a = _run(data)
    b = _run(data, densify_by="grad", revised_opacity=False)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[4].error_passes == [] and a[4].densify_by == "grad" and sorted(a[3]) == list(REFINING)
    # the other fields are idle under "grad"
    c = _run(data, densify_error_thresh=0.0, densify_error_views=1, densify_growth=1.0, densify_max_splats=0)
    assert a[0] == c[0] and np.array_equal(a[1], c[1])


def _tiny_splats(dev, n=12, seed=3):
    import torch

    import brush_amd

    rng = np.random.default_rng(seed)
    means = np.c_[rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(-0.5, 0.5, n)].astype(np.float32)
    log_scales = np.full((n, 3), math.log(0.1), np.float32)
    log_scales[3] = math.log(0.001)  # below densify_size_thresh: cloned; the others are split
    raw_opac = rng.uniform(-1.0, 2.0, n).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.uniform(0.0, 1.0, (n, 1, 3)).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=dev)
    return brush_amd.Splats(t(means), t(sh), t(quats), t(raw_opac), t(log_scales))


def test_refining_without_scores_is_refused(dev):
    import torch

    import brush_amd
    from brush_amd import SplatTrainer, TrainConfig

    splats = _tiny_splats(dev)
    n = splats.num_splats()
    cam = brush_amd.Camera([0.0, 0.0, -6.0], [0.0, 0.0, 0.0, 1.0], 0.6, 0.5, (0.5, 0.5))
    gt = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    tr = SplatTrainer(splats, TrainConfig(densify_by="error", warmup_steps=0, refine_every=2, densify_error_thresh=0.5,
                                          densify_growth=1.0))
    assert not tr.will_refine()
    tr.step(splats, cam, gt)
    assert tr.will_refine() and tr.iter == 1
    before = splats.means.detach().clone()
    with pytest.raises(ValueError, match=r"no scores for this refinement: call set_densify_scores first"):
        tr.step(splats, cam, gt)
    tr.set_densify_scores(torch.ones(n + 1, device=dev))
    with pytest.raises(ValueError, match=r"stale densification scores: 13 scores for 12 splats.*set_densify_scores"):
        tr.step(splats, cam, gt)
    assert tr.iter == 1 and tr.opt_time == 1 and torch.equal(before, splats.means.detach())  # nothing was stepped
    with pytest.raises(ValueError, match="float32"):
        tr.set_densify_scores(torch.ones(n, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="on the GPU"):
        tr.set_densify_scores(torch.ones(n))
    scores = torch.zeros(n, device=dev)
    scores[[3, 7]] = 1.0
    tr.set_densify_scores(scores)
    tr.step(splats, cam, gt)
    assert tr.densify_scores is None  # consumed
    assert (tr.last_refine.num_cloned, tr.last_refine.num_split) == (1, 1)
    assert not tr.grad_2d_accum.any() and not tr.xy_grad_counts.any()  # the statistics are not gathered
    # direct callers of refine_splats are told the same
    with pytest.raises(ValueError, match="set_densify_scores"):
        tr.refine_splats(splats, {})
    # and the step's refusals
    for kw, what in (({"grad_sync": lambda block, aux: None}, "exchange / grad_sync"), ({"exposures": object(),
                                                                                         "view_index": 0},
                                                                                        "exposure compensation"),
                     ({"poses": object(), "view_index": 0}, "pose refinement")):
        with pytest.raises(ValueError, match=f"densify_by='error' cannot be combined with {what}"):
            tr.step(splats, cam, gt, **kw)


def test_revised_opacity_changes_only_the_documented_rows(dev):
    import torch

    from brush_amd import SplatTrainer, TrainConfig
    from brush_amd.train import revised_opacity

    out = {}
    for flag in (False, True):
        splats = _tiny_splats(dev)
        n = splats.num_splats()
        tr = SplatTrainer(splats, TrainConfig(densify_by="error", revised_opacity=flag, refine_every=4,
                                              densify_error_thresh=0.5, densify_growth=1.0, cull_alpha_thresh=0.0,
                                              seed=5))
        tr.iter = 5  # (5 // 4) % 30 != 0: no opacity reset at this refinement
        scores = torch.zeros(n, device=dev)
        scores[[3, 7]] = 1.0
        tr.set_densify_scores(scores)
        post_opac = splats.raw_opacity.detach().clone()
        pre = {"means": splats.means.detach() + 0.01, "rotation": splats.rotation.detach().clone(),
               "sh": splats.sh_coeffs.detach().clone(), "opac": post_opac - 0.25,
               "scales": splats.log_scales.detach().clone()}
        st = tr.refine_splats(splats, pre)
        assert (st.num_cloned, st.num_split, st.num_transparent_pruned, st.num_scale_pruned) == (1, 1, 0, 0)
        assert splats.num_splats() == n + 2
        out[flag] = {k: getattr(splats, k).detach().clone() for k in
                     ("means", "sh_coeffs", "rotation", "raw_opacity", "log_scales")}
    n = 12
    for k in ("means", "sh_coeffs", "rotation", "log_scales"):
        assert torch.equal(out[False][k], out[True][k]), k
    a, b = out[False]["raw_opacity"], out[True]["raw_opacity"]
    rows = [3, 7, n, n + 1]  # the clone source, the split source, the clone, the split
    others = [i for i in range(n + 2) if i not in rows]
    assert torch.equal(a[others], b[others])
    want = revised_opacity(post_opac[[3, 7]])  # from the sources' POST-step opacities
    assert torch.equal(b[[3, 7]], want) and torch.equal(b[[n, n + 1]], want)
    assert torch.equal(a[:n], post_opac) and torch.equal(a[n], post_opac[3] - 0.25) and torch.equal(a[n + 1], post_opac[7])
    assert bool((b[rows] < a[rows]).all())


def test_revised_opacity_under_the_gradient_rule(dev, data, deterministic):
    """The option applies under densify_by="grad" too: same run up to the first refinement, then other opacities."""
    a = _run(data, steps=7, densify_grad_thresh=0.0)  # (a zero threshold: every splat with a gradient densifies)
    b = _run(data, steps=7, densify_grad_thresh=0.0, revised_opacity=True)
    assert np.array_equal(a[1][:6], b[1][:6]) and a[2][:5] == b[2][:5]
    st = a[3][5][1]
    assert st.num_split + st.num_cloned > 0 and not np.array_equal(a[1][6:], b[1][6:])


def test_command_line_round_trip(scene_dir, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    log_json = str(tmp_path / "log.json")
    r = subprocess.run([sys.executable, "-m", "brush_amd.train_loop", scene_dir, "--steps", "8", "--init-count", "400",
                        "--sh-degree", "1", "--densify-by", "error", "--densify-error-thresh", "0.25",
                        "--densify-error-views", "2", "--densify-growth", "0.1", "--max-splats", "5000",
                        "--revised-opacity", "--json", log_json], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(log_json) as f:
        log = json.load(f)
    assert log["densify_by"] == "error" and log["error_passes"] == []  # 8 steps: inside the default warm-up
    assert (log["densify_error_thresh"], log["densify_error_views"], log["densify_growth"], log["max_splats"],
            log["revised_opacity"]) == (0.25, 2, 0.1, 5000, True)
    assert log["steps"] == 8 and len(log["losses"]) == 8 and np.isfinite(log["losses"]).all()
