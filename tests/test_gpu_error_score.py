"""GPU checks of the per-splat error replay (brush_render_error_scores, brush_l1_error_map, brush_amd/error_score.py):
the hand-made kernel inputs of tests/contrib_cases.py under seeded error maps against the float64 reference of
tests/error_ref64.py, the all-ones map against the contribution replay bit for bit, zero, one-hot and out-of-range
maps, wrong references rejected, the fold across views and repeatability, the L1 error map by bits, and a rendered
scene through splat_error_scores."""
import functools
import math

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import error_ref64 as R
from tests import helpers as H
from tests import margins

pytestmark = pytest.mark.gpu

CASES = CC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
Q24 = 2.0 ** 24


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def random_map(case, seed=0):
    """A seeded float32 map in [0, 1] of the case's frame."""
    rng = np.random.default_rng(1000 + seed + 7 * case["w"] + case["h"])
    return rng.uniform(0.0, 1.0, (case["h"], case["w"])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref_random(name):
    """One reference walk per case under its seeded map, shared and left unchanged."""
    return R.walk(BY_NAME[name], random_map(BY_NAME[name]))


def _aux(case, dev):
    """The case's arrays as a RenderAux; what the entries do not read are one-word dummies."""
    import torch

    from brush_amd import _lib
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
    return u, aux


def _run(case, dev, *maps):
    """The kernel on a hand-made case, one call and fold per map; returns the ErrorScoreBuffers."""
    import torch

    from brush_amd.error_score import ErrorScoreBuffers, error_scores_from_aux

    u, aux = _aux(case, dev)
    bufs = ErrorScoreBuffers(case["n"], dev)
    for m in maps:
        error_scores_from_aux(u, aux, torch.as_tensor(np.ascontiguousarray(m, np.float32), device=dev), bufs)
    return bufs


def _ints(case, dev, m):
    """The per-splat integers of one call."""
    return _run(case, dev, m).score_sum[:case["n"]].cpu().numpy()


# ---------------------------------------------------------------------------- 1. the gate
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gate_against_the_reference(dev, case):
    ref = ref_random(case["name"])
    got = _ints(case, dev, random_map(case))
    ratio = R.gate(got / Q24, ref)
    print(f"{case['name']}: touched {int(ref['touched'].sum())} err/tol {ratio:.4f}")
    margins.record("error_score", "err", ratio)
    assert ratio <= 1.0, ratio
    margins.check_growth("error_score", "err", ratio)
    assert not got[~ref["touched"]].any()  # rows the reference never touches stay zero


# ---------------------------------------------------------------------------- 2. all ones: the contribution replay
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_all_ones_map_is_the_contribution_sum(dev, case):
    from brush_amd.contribution import ContributionBuffers, contributions_from_aux

    got = _ints(case, dev, np.ones((case["h"], case["w"]), np.float32))
    u, aux = _aux(case, dev)
    cb = ContributionBuffers(case["n"], dev)
    contributions_from_aux(u, aux, None, cb, check=False)
    want = cb.counts[:case["n"], 0].cpu().numpy()
    assert np.array_equal(got, want)
    assert case["num_isect"] == 0 or want.any()


# ---------------------------------------------------------------------------- 3. all zeros
@pytest.mark.parametrize("name", ["one_record", "batch_65", "ragged_17x9", "random_200"])
def test_all_zeros_map_leaves_every_buffer_zero(dev, name):
    case = BY_NAME[name]
    b = _run(case, dev, np.zeros((case["h"], case["w"]), np.float32))
    for t in (b.view_err, b.score_max, b.score_sum, b.views_seen):
        assert not t.any()
    assert b.views == 1


# ---------------------------------------------------------------------------- 4. one-hot maps
@pytest.mark.parametrize("name", ["ragged_17x9", "random_200"])
def test_one_hot_maps(dev, name):
    case = BY_NAME[name]
    w, h = case["w"], case["h"]
    some_hit = 0
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 3), (w - 1, h // 2), (5, h - 1)):
        m = np.zeros((h, w), np.float32)
        m[y, x] = 1.0
        ref = R.walk(case, m)
        got = _ints(case, dev, m)
        ratio = R.gate(got / Q24, ref)
        assert ratio <= 1.0, (x, y, ratio)
        assert not got[ref["err"] == 0].any(), (x, y)  # splats that do not hit the pixel
        some_hit += int((got != 0).sum())
    assert some_hit > 0


# ---------------------------------------------------------------------------- 5. out-of-range values
@pytest.mark.parametrize("name", ["ragged_17x9", "random_200", "batch_129"])
def test_out_of_range_values_are_clamped(dev, name):
    case = BY_NAME[name]
    m = random_map(case, seed=5)
    flat = m.reshape(-1)
    bad = np.array([-1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    idx = np.random.default_rng(3).permutation(flat.size)[:5 * (flat.size // 10)]
    flat[idx] = np.tile(bad, idx.size // 5)
    twin = R.clamp_map(m).astype(np.float32)
    assert np.isnan(m).any() and not np.isnan(twin).any() and twin.min() == 0.0 and twin.max() == 1.0
    got, want = _ints(case, dev, m), _ints(case, dev, twin)
    assert np.array_equal(got, want) and want.any()


# ---------------------------------------------------------------------------- 6. wrong references
def wide_map(case):
    """A seeded map in [-1, 2]: a third of it below 0, a third above 1 (what `unclamped` gets wrong)."""
    rng = np.random.default_rng(77 + case["w"])
    return rng.uniform(-1.0, 2.0, (case["h"], case["w"])).astype(np.float32)


@pytest.mark.parametrize("mutation,name,make_map", [
    ("ignore_map", "random_200", random_map), ("transposed_map", "ragged_17x9", random_map),
    ("transposed_map", "random_200", random_map), ("unclamped", "random_200", wide_map),
    ("ignore_T", "random_200", random_map)])
def test_each_wrong_reference_fails_the_gate(dev, mutation, name, make_map):
    case = BY_NAME[name]
    m = make_map(case)
    ref, wrong = R.walk(case, m), R.walk(case, m, mutate=mutation)
    assert not R.passes(R.gate(ref["err"], wrong))  # on the CPU first: the case separates the mutant
    got = _ints(case, dev, m) / Q24
    assert R.passes(R.gate(got, ref))
    assert not R.passes(R.gate(got, wrong)), (mutation, name)


# ---------------------------------------------------------------------------- 7. accumulation, repeatability, aux modes
def test_views_fold_and_runs_repeat_bitwise(dev):
    case = BY_NAME["random_200"]
    m1, m2 = random_map(case, seed=1), random_map(case, seed=2)
    m2[:, :24] = 0.0  # some splats see an error in one view only
    a, b = _ints(case, dev, m1), _ints(case, dev, m2)
    both = _run(case, dev, m1, m2)
    n = case["n"]
    assert both.views == 2 and not both.view_err.any()
    assert np.array_equal(both.score_max[:n].cpu().numpy(), np.maximum(a, b))
    assert np.array_equal(both.score_sum[:n].cpu().numpy(), a + b)
    seen = (a != 0).astype(np.int32) + (b != 0).astype(np.int32)
    assert np.array_equal(both.views_seen[:n].cpu().numpy(), seen) and set(np.unique(seen)) == {0, 1, 2}
    again = _run(case, dev, m1, m2)
    for k in ("score_max", "score_sum", "views_seen"):
        assert np.array_equal(getattr(both, k).cpu().numpy(), getattr(again, k).cpu().numpy()), k
    # scores(): int64 -> float64 / 2^24 -> float32, on the device
    want_max, want_sum = np.maximum(a, b).astype(np.float64) / Q24, (a + b).astype(np.float64) / Q24
    assert np.array_equal(both.scores("max").cpu().numpy(), want_max.astype(np.float32))
    assert np.array_equal(both.scores("sum").cpu().numpy(), want_sum.astype(np.float32))
    assert np.array_equal(both.scores("mean").cpu().numpy(), (want_sum / np.maximum(seen, 1)).astype(np.float32))
    r = both.read()
    assert r.views == 2 and np.array_equal(r.max.numpy(), want_max) and np.array_equal(r.sum.numpy(), want_sum)
    assert np.array_equal(r.views_seen.numpy(), seen)
    with pytest.raises(ValueError, match="by must be"):
        both.scores("median")


def _camera(w, h, position=None):
    import brush_amd

    c = H.reference_test_camera(w, h)
    return brush_amd.Camera(position or c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def test_deterministic_and_default_aux_modes_agree_bitwise(dev):
    import torch

    import brush_amd
    from brush_amd import render as Rn
    from brush_amd.error_score import ErrorScoreBuffers, error_scores_from_aux

    d = H.load_case("basic_case")
    w, h = 50, 41
    splats = brush_amd.Splats.from_safetensors(d, dev)
    emap = torch.as_tensor(np.random.default_rng(8).uniform(0, 1, (h, w)).astype(np.float32), device=dev)
    out = []
    with torch.no_grad():
        rot = splats.rotation.detach()
        norm_rot = (rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))).contiguous()
        for det in (False, True, False):
            _, aux, u = Rn._forward_impl(_camera(w, h), (w, h), splats.means.detach(), splats.log_scales.detach(),
                                         norm_rot, splats.sh_coeffs.detach(), splats.raw_opacity.detach(), False, None,
                                         deterministic=det, expect_backward=False)
            bufs = ErrorScoreBuffers(splats.num_splats(), dev)
            error_scores_from_aux(u, aux, emap, bufs)
            out.append(bufs.score_sum.cpu().numpy())
    assert out[0].any() and np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    with pytest.raises(ValueError, match="error_map must be"):
        error_scores_from_aux(u, aux, emap.t().contiguous(), bufs)  # [w,h]
    with pytest.raises(ValueError, match="error_map must be"):
        error_scores_from_aux(u, aux, emap.double(), bufs)


# ---------------------------------------------------------------------------- 8. the L1 error map
def l1_map_f32(pred, gt, mask):
    """numpy float32 restatement: min(((|dr| + |dg|) + |db|) * (1/3), 1), 0 under the mask."""
    f32 = np.float32
    g = gt.astype(f32) / f32(255.0) if gt.dtype == np.uint8 else gt.astype(f32)
    d = [np.abs(pred[..., k].astype(f32) - g[..., k]) for k in range(3)]
    out = np.minimum(((d[0] + d[1]) + d[2]) * (f32(1.0) / f32(3.0)), f32(1.0)).astype(f32)
    return out if mask is None else np.where(mask != 0, out, f32(0.0)).astype(f32)


@pytest.mark.parametrize("size", [(17, 9), (48, 32)])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
def test_l1_error_map_by_bits(dev, size, u8, channels, masked):
    import torch

    from brush_amd.error_score import l1_error_map

    w, h = size
    rng = np.random.default_rng(w * 100 + channels * 10 + int(u8) * 2 + int(masked))
    pred = rng.uniform(-0.2, 1.6, (h, w, 4)).astype(np.float32)  # beyond [0, 1]: the clamp at 1 is reached
    gt = rng.integers(0, 256, (h, w, channels)).astype(np.uint8) if u8 \
        else rng.uniform(0, 1, (h, w, channels)).astype(np.float32)
    pred[0, 0, :3] = 3.0  # a pixel whose mean difference is above 1
    mask = (rng.uniform(0, 1, (h, w)) < 0.6).astype(np.uint8) * 255 if masked else None
    if masked:
        mask[0, 0] = 255
    want = l1_map_f32(pred, gt, mask)
    got = l1_error_map(torch.as_tensor(pred, device=dev), torch.as_tensor(gt, device=dev),
                       None if mask is None else torch.as_tensor(mask, device=dev))
    assert got.shape == (h, w) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert want[0, 0] == 1.0 and 0.0 < want.mean() < 1.0
    out = torch.full((h, w), -1.0, device=dev)
    assert l1_error_map(torch.as_tensor(pred, device=dev), torch.as_tensor(gt, device=dev),
                        None if mask is None else torch.as_tensor(mask, device=dev), out=out) is out
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_l1_error_map_refuses_bad_arguments(dev):
    import torch

    from brush_amd.error_score import l1_error_map

    pred = torch.zeros((9, 17, 4), device=dev)
    gt = torch.zeros((9, 17, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="pred must be"):
        l1_error_map(pred[..., :3], gt)
    with pytest.raises(ValueError, match="gt must be"):
        l1_error_map(pred, gt[:8])
    with pytest.raises(ValueError, match="uint8 or float32"):
        l1_error_map(pred, gt.to(torch.int32))
    with pytest.raises(ValueError, match="mask must be"):
        l1_error_map(pred, gt, torch.zeros((9, 17), device=dev))
    with pytest.raises(ValueError, match="out must be"):
        l1_error_map(pred, gt, out=torch.zeros((17, 9), device=dev))


# ---------------------------------------------------------------------------- 9. a rendered scene
W9, H9 = 64, 48


@pytest.fixture(scope="module")
def scene(dev):
    """Seeded: 900 splats in a box in front of three cameras, and three targets rendered from a perturbed copy (so the
    L1 error is neither zero nor saturated).  Device-resident (Camera, gt u8, mask or None) triples."""
    import torch

    import brush_amd

    rng = np.random.default_rng(31)
    n = 900
    means = np.c_[rng.uniform(-2.5, 2.5, (n, 2)), rng.uniform(-1.0, 1.0, n)].astype(np.float32)
    log_scales = np.full((n, 3), math.log(0.12), np.float32) + rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    raw_opac = rng.uniform(-1.0, 2.0, n).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.uniform(-0.5, 1.5, (n, 1, 3)).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=dev)
    splats = brush_amd.Splats(t(means), t(sh), t(quats), t(raw_opac), t(log_scales))
    other = brush_amd.Splats(t(means + rng.normal(0, 0.05, means.shape).astype(np.float32)), t(sh[::-1].copy()),
                             t(quats), t(raw_opac), t(log_scales))
    cams = [brush_amd.Camera(p, [0.0, 0.0, 0.0, 1.0], 0.6, 0.6 * H9 / W9, (0.5, 0.5))
            for p in ([-1.0, 0.0, -8.0], [1.0, 0.2, -8.0], [0.0, -0.5, -7.0])]
    views = []
    with torch.no_grad():
        for k, cam in enumerate(cams):
            img, _ = other.render(cam, (W9, H9), False)
            gt = (img[..., :3].clamp(0, 1) * 255.0).round().to(torch.uint8).contiguous()
            mask = None
            if k == 1:
                mask = torch.ones((H9, W9), dtype=torch.uint8, device=dev)
                mask[:, :20] = 0
            views.append((cam, gt, mask))
    torch.cuda.synchronize()
    return splats, views


def test_rendered_scene_ones_error_is_the_contribution_sum(dev, scene):
    import torch

    from brush_amd import splat_contributions, splat_error_scores

    splats, views = scene
    ones = lambda p, g: torch.ones(p.shape[:2], dtype=torch.float32, device=p.device)
    bufs = splat_error_scores(splats, views, use_masks=False, error=ones)
    c = splat_contributions(splats, [(cam, (W9, H9)) for cam, _, _ in views])
    got = bufs.read()
    assert got.views == 3 and float(c.sum.sum()) > 100.0
    assert np.array_equal(got.sum.numpy() * Q24, c.sum.numpy() * Q24)
    assert np.array_equal(bufs.score_sum[:bufs.n].cpu().numpy(), np.rint(c.sum.numpy() * Q24).astype(np.int64))
    # antialiased: the same identity in that mode
    aa = splat_error_scores(splats, views[:1], use_masks=False, error=ones, antialiased=True).read()
    c_aa = splat_contributions(splats, [(views[0][0], (W9, H9))], antialiased=True)
    assert np.array_equal(aa.sum.numpy(), c_aa.sum.numpy()) and not np.array_equal(aa.sum.numpy(), got.sum.numpy())


def test_rendered_scene_l1_path_repeats_and_honours_options(dev, scene):
    import torch

    from brush_amd import splat_error_scores
    from brush_amd.compose import as_background

    splats, views = scene
    a, b = splat_error_scores(splats, views), splat_error_scores(splats, views)
    for k in ("score_max", "score_sum", "views_seen"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), k
    assert a.views == 3 and a.score_sum.any() and int(a.views_seen.max()) == 3
    r = a.read()
    assert float(r.max.max()) > 0.0 and (r.max <= r.sum).all()
    # the mask of view 1 takes error away; without masks the sum can only be larger
    unmasked = splat_error_scores(splats, views, use_masks=False)
    assert (unmasked.score_sum >= a.score_sum).all() and (unmasked.score_sum > a.score_sum).any()
    # a background changes what the error is measured on (a bright colour under a dark scene: more error)
    white = splat_error_scores(splats, views, background=as_background("white", dev))
    assert not np.array_equal(white.score_sum.cpu().numpy(), a.score_sum.cpu().numpy())
    with pytest.raises(ValueError, match="random"):
        splat_error_scores(splats, views, background="random")


def test_score_pass_with_resident_views_does_not_synchronise(dev, scene):
    import torch

    from brush_amd import splat_error_scores
    from brush_amd.compose import as_background

    splats, views = scene
    bg = as_background((0.2, 0.3, 0.4), dev)
    splat_error_scores(splats, views, background=bg)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.zeros(1, device=dev).item()  # the mode sees a read-back
        bufs = splat_error_scores(splats, views, background=bg)
        plain = splat_error_scores(splats, views)
        scores = bufs.scores("max"), plain.scores("mean")
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(bool(torch.isfinite(s).all()) for s in scores) and bool(scores[0].any())
