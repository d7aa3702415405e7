"""GPU checks of the feature replays (brush_render_features, brush_render_features_backward,
brush_render_feature_sums, brush_amd/features.py): the hand-made kernel inputs of tests/contrib_cases.py against the
float64 reference of tests/features_ref64.py at C in {1, 3, 4, 5, 16, 17, 64} (a lone channel, non-multiples of 4, a
full pass, a pass boundary plus one, the cap); exact identities with the forward's depth and colour, the error replay
and the contribution replay; the label kind against its one-hot maps; the adjoint identity; autograd; wrong references
rejected; label lifting on a rendered scene of two groups; refusals.

k_rasterize_quad's epilogue stores its colour accumulators unchanged (make_float4(cr, cg, cb_, 1 - T), no clamp, no
background), and accumulates them as c = fmaf(colour, fac, c) under the pixel's own predicate: so the drawn colours
(words 5..7 of a projected row) as features must reproduce img[..., :3] bit for bit, as compact_depth reproduces
out_depth."""
import functools
import os

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import features_ref64 as R

pytestmark = pytest.mark.gpu

CASES = CC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
CHANNELS = (1, 3, 4, 5, 16, 17, 64)
Q24 = 2.0 ** 24
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def ref(name, c):
    """(features, v, maps, reference walk) of a case at C = c: computed once, shared and left unchanged."""
    f, v, m = R.seeded(BY_NAME[name], c)
    return f, v, m, R.walk(BY_NAME[name], f, v, m)


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


def _t(a, dev):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def fwd(case, dev, f):
    from brush_amd.features import features_from_aux

    u, aux = _aux(case, dev)
    return features_from_aux(u, aux, _t(f, dev)).cpu().numpy()


def grads(case, dev, v, c, into=None):
    import torch

    from brush_amd.features import feature_grads_from_aux

    u, aux = _aux(case, dev)
    g = torch.zeros((case["n"], c), dtype=torch.float32, device=dev) if into is None else _t(into, dev)
    return feature_grads_from_aux(u, aux, _t(v, dev), g).cpu().numpy()


def sums(case, dev, c, *maps):
    import torch

    from brush_amd.features import feature_sums_from_aux

    u, aux = _aux(case, dev)
    s = torch.zeros((case["n"], c), dtype=torch.int64, device=dev)
    for m in maps:
        feature_sums_from_aux(u, aux, _t(m, dev), s)
    return s.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_gate_zeros_and_repeatability(dev, case):
    for c in CHANNELS:
        f, _, _, want = ref(case["name"], c)
        got = fwd(case, dev, f)
        assert got.shape == (case["h"], case["w"], c) and got.dtype == np.float32
        r = R.gate(want, out=got)["out"]
        print(f"{case['name']} C={c}: forward err/tol {r:.4f}")
        assert r <= 1.0, (c, r)
        assert not bits(got[~want["added"]]).any(), c  # exactly +0 where the reference adds nothing
        assert np.array_equal(bits(got), bits(fwd(case, dev, f))), c
    assert case["num_isect"] == 0 or want["added"].any()


def test_forward_writes_every_pixel_of_a_prefilled_output_and_n_zero(dev):
    import torch

    from brush_amd.features import features_from_aux

    case = BY_NAME["ragged_17x9"]
    for c in (5, 16):
        f, _, _, want = ref(case["name"], c)
        u, aux = _aux(case, dev)
        out = torch.full((case["h"], case["w"], c), float("nan"), device=dev)
        assert features_from_aux(u, aux, _t(f, dev), out=out) is out
        assert R.gate(want, out=out.cpu().numpy())["out"] <= 1.0
        # no splats: zeros everywhere, no list is read
        out.fill_(float("nan"))
        features_from_aux(u, aux, torch.zeros((0, c), device=dev), out=out)
        assert not bits(out.cpu().numpy()).any()


# ---------------------------------------------------------------------------- 2. exact identities on a rendered scene
def _camera(w, h, position=(0.0, 0.0, -8.0)):
    import brush_amd

    return brush_amd.Camera(list(position), [0.0, 0.0, 0.0, 1.0], 0.6, 0.6 * h / w, (0.5, 0.5))


N_GROUP, N_OFF = 90, 12


@pytest.fixture(scope="module")
def scene(dev):
    """Seeded: two spatially separated groups of 90 opaque splats (ids [0, 90): left, [90, 180): right) and 12 far
    outside every frame (ids 180..191)."""
    import torch

    import brush_amd

    rng = np.random.default_rng(52)
    n = 2 * N_GROUP + N_OFF
    means = np.zeros((n, 3), np.float32)
    means[:N_GROUP, 0] = rng.uniform(-1.9, -0.8, N_GROUP)
    means[N_GROUP:2 * N_GROUP, 0] = rng.uniform(0.8, 1.9, N_GROUP)
    means[:2 * N_GROUP, 1] = rng.uniform(-1.0, 1.0, 2 * N_GROUP)
    means[:2 * N_GROUP, 2] = rng.uniform(-0.5, 0.5, 2 * N_GROUP)
    means[2 * N_GROUP:] = np.c_[rng.uniform(40.0, 60.0, N_OFF), rng.uniform(40.0, 60.0, N_OFF), np.zeros(N_OFF)]
    log_scales = (np.log(0.25) + rng.uniform(-0.15, 0.15, (n, 3))).astype(np.float32)
    raw_opac = rng.uniform(3.0, 5.0, n).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.uniform(-0.5, 1.5, (n, 1, 3)).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=dev)
    return brush_amd.Splats(t(means), t(sh), t(quats), t(raw_opac), t(log_scales))


def _parts(splats):
    import torch

    with torch.no_grad():
        rot = splats.rotation.detach()
        norm_rot = (rot / torch.sqrt(torch.sum(rot * rot, dim=1, keepdim=True))).contiguous()
    return (splats.means.detach(), splats.log_scales.detach(), norm_rot, splats.sh_coeffs.detach(),
            splats.raw_opacity.detach())


@pytest.mark.parametrize("size", [(48, 32), (17, 9)])
def test_depth_and_colour_identities_and_aux_modes(dev, scene, size):
    import torch

    from brush_amd import render as Rn
    from brush_amd.features import features_from_aux

    w, h = size
    n = scene.num_splats()
    outs = []
    with torch.no_grad():
        for det in (False, True):
            depth = Rn._depth_buffers(n, (w, h), dev)
            img, aux, u = Rn._forward_impl(_camera(w, h), (w, h), *_parts(scene), False, None, deterministic=det,
                                           expect_backward=False, depth=depth)
            nvis = int(aux.num_visible.cpu()[0])
            g = aux.global_from_compact_gid[:nvis].long()
            feats = torch.zeros((n, 4), device=dev)
            feats[g, 0] = depth[1][:nvis]                   # z, scattered to global ids
            feats[g, 1:4] = aux.projected_splats[:nvis, 5:8]  # the colours the forward drew
            out = features_from_aux(u, aux, feats)
            assert nvis >= 2 * N_GROUP - 5 and float(img[..., 3].max()) > 0.9
            assert np.array_equal(bits(out[..., 0].cpu().numpy()), bits(depth[0].cpu().numpy()))
            assert np.array_equal(bits(out[..., 1:4].cpu().numpy()), bits(img[..., :3].cpu().numpy()))
            # the same through a pass of one channel (scalar loads and stores)
            one = features_from_aux(u, aux, feats[:, :1].contiguous())
            assert np.array_equal(bits(one[..., 0].cpu().numpy()), bits(depth[0].cpu().numpy()))
            rng = np.random.default_rng(9)
            f17 = _t(rng.uniform(-1, 1, (n, 17)).astype(np.float32), dev)
            m17 = _t(rng.uniform(0, 1, (h, w, 17)).astype(np.float32), dev)
            s17 = torch.zeros((n, 17), dtype=torch.int64, device=dev)
            from brush_amd.features import feature_sums_from_aux

            feature_sums_from_aux(u, aux, m17, s17)
            outs.append((features_from_aux(u, aux, f17).cpu().numpy(), s17.cpu().numpy()))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and outs[0][0].any()
    assert np.array_equal(outs[0][1], outs[1][1]) and outs[0][1].any()


# ---------------------------------------------------------------------------- 3. the exact sums
def seeded_map(case, seed=0):
    rng = np.random.default_rng(1000 + seed + 7 * case["w"] + case["h"])
    return rng.uniform(0.0, 1.0, (case["h"], case["w"])).astype(np.float32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_channel_sums_are_the_error_scores_and_ones_the_contribution_sum(dev, case):
    import torch

    from brush_amd.contribution import ContributionBuffers, contributions_from_aux
    from brush_amd.error_score import ErrorScoreBuffers, error_scores_from_aux

    u, aux = _aux(case, dev)
    m = seeded_map(case)
    eb = ErrorScoreBuffers(case["n"], dev)
    error_scores_from_aux(u, aux, _t(m, dev), eb)
    want = eb.score_sum[:case["n"]].cpu().numpy()
    got = sums(case, dev, 1, m[..., None])
    assert np.array_equal(got[:, 0], want)
    assert case["num_isect"] == 0 or want.any()
    cb = ContributionBuffers(case["n"], dev)
    contributions_from_aux(u, aux, None, cb, check=False)
    contrib = cb.counts[:case["n"], 0].cpu().numpy()
    for c in CHANNELS:
        got = sums(case, dev, c, np.ones((case["h"], case["w"], c), np.float32))
        assert np.array_equal(got, np.repeat(contrib[:, None], c, axis=1)), c


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sums_gate_and_accumulation(dev, case):
    for c in CHANNELS:
        _, _, m, want = ref(case["name"], c)
        got = sums(case, dev, c, m)
        r = R.gate(want, q=got / Q24)["q"]
        print(f"{case['name']} C={c}: sums err/tol {r:.4f}")
        assert r <= 1.0, (c, r)
        assert not got[~want["touched"]].any(), c
        assert np.array_equal(sums(case, dev, c, m, m), 2 * got), c  # two calls accumulate exactly


@pytest.mark.parametrize("name", ["ragged_17x9", "four_tiles", "random_200", "batch_129"])
def test_label_kind_is_the_one_hot_f32_kind(dev, name):
    case = BY_NAME[name]
    rng = np.random.default_rng(3 + case["w"])
    for c in CHANNELS:
        labels = rng.integers(0, c + 3, (case["h"], case["w"])).astype(np.uint8)  # c, c + 1, c + 2: no class
        labels[rng.uniform(size=labels.shape) < 0.1] = 255
        labels[0, 0], labels[-1, -1] = 255, c
        hot = R.one_hot(labels, c)
        assert hot.shape[2] == c and not hot[labels >= c].any()
        got, want = sums(case, dev, c, labels), sums(case, dev, c, hot)
        assert np.array_equal(got, want), c
        assert want.any()


@pytest.mark.parametrize("name", ["ragged_17x9", "random_200", "batch_129"])
def test_out_of_range_map_values_are_clamped(dev, name):
    from tests.error_ref64 import clamp_map

    case = BY_NAME[name]
    for c in (1, 5, 17):
        m = R.seeded(case, c, seed=5)[2]
        flat = m.reshape(-1)
        bad = np.array([-1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
        idx = np.random.default_rng(3).permutation(flat.size)[:5 * (flat.size // 10)]
        flat[idx] = np.tile(bad, idx.size // 5)
        twin = clamp_map(m).astype(np.float32)
        assert np.isnan(m).any() and not np.isnan(twin).any() and twin.min() == 0.0 and twin.max() == 1.0
        got, want = sums(case, dev, c, m), sums(case, dev, c, twin)
        assert np.array_equal(got, want) and want.any(), c


# ---------------------------------------------------------------------------- 4. the float transpose
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_transpose_gate_adjoint_and_accumulation(dev, case):
    n = case["n"]
    for c in CHANNELS:
        f, v, _, want = ref(case["name"], c)
        got = grads(case, dev, v, c)
        r = R.gate(want, grad=got)["grad"]
        print(f"{case['name']} C={c}: transpose err/tol {r:.4f}")
        assert r <= 1.0, (c, r)
        assert not bits(got[~want["touched"]]).any(), c  # rows the reference never touches stay exactly zero
        # <out(f), v> = <f, v_f(v)>, in float64 on the GPU's outputs, within what the two allowances imply
        out = fwd(case, dev, f).astype(np.float64)
        lhs, rhs = float((out * v).sum()), float((f.astype(np.float64) * got).sum())
        bound = float((np.abs(v) * want["tol_out"]).sum() + (np.abs(f) * want["tol_grad"]).sum())
        assert abs(lhs - rhs) <= bound, (c, lhs, rhs, bound)
        # the entry accumulates into what is there
        base = np.random.default_rng(c).normal(size=(n, c)).astype(np.float32)
        acc = grads(case, dev, v, c, into=base)
        # (every partial sum added to the row rounds once more, at the magnitude of base + what has arrived)
        tol = want["tol_grad"] + R.U * (np.abs(base) + want["abs_grad"]) * (1.0 + want["partials"])[:, None]
        assert R.ratio(acc, base.astype(np.float64) + want["grad"], tol) <= 1.0, c
        assert np.array_equal(bits(acc[~want["touched"]]), bits(base[~want["touched"]])), c


# ---------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("size", [(48, 32), (17, 9)])
def test_autograd_is_the_bare_transpose_and_img_carries_no_graph(dev, scene, size):
    import torch

    from brush_amd.features import feature_grads_from_aux

    w, h = size
    n = scene.num_splats()
    rng = np.random.default_rng(w)
    for c in (3, 17):
        feats = _t(rng.uniform(-1, 1, (n, c)).astype(np.float32), dev).requires_grad_(True)
        v = _t(rng.normal(size=(h, w, c)).astype(np.float32), dev)
        img, feat, aux = scene.render_features(_camera(w, h), (w, h), feats)
        assert feat.shape == (h, w, c) and feat.requires_grad and feat.grad_fn is not None
        assert not img.requires_grad and img.grad_fn is None and img.shape == (h, w, 4)
        g, = torch.autograd.grad((feat * v).sum(), feats)
        from brush_amd.render import pack_uniforms

        u = pack_uniforms(_camera(w, h), (w, h), 0, n)
        bare = torch.zeros((n, c), device=dev)
        feature_grads_from_aux(u, aux, v, bare)
        # Both are sums of the SAME float32 products fac v (the walk is bitwise repeatable), added in different orders
        # by the atomics.  Each differs from the exact sum of those products by at most (6 + P) U S, S = sum |fac v|
        # (the F32 allowance's summation term), P <= 4 quadrants x tiles partial sums per row; S is the transpose of
        # |v|, itself known to 1 + (6 + P) U.
        absg = torch.zeros((n, c), device=dev)
        feature_grads_from_aux(u, aux, v.abs(), absg)
        depth = R.K_TREE + 4 * ((w + 15) // 16) * ((h + 15) // 16)
        tol = 2.0 * depth * R.U * absg.double().cpu().numpy() * (1.0 + 2.0 * depth * R.U)
        assert R.ratio(g.cpu().numpy(), bare.double().cpu().numpy(), tol) <= 1.0, c
        assert bool(g.any()) and not bool(g[2 * N_GROUP:].any())  # the splats outside the frame receive nothing
        assert all(p.grad is None for p in (scene.means, scene.log_scales, scene.raw_opacity))


# ---------------------------------------------------------------------------- 6. wrong references
@pytest.mark.parametrize("mutation,name", [
    ("chw", "ragged_17x9"), ("chw", "random_200"), ("channel_off_by_one", "batch_65"), ("ignore_T", "random_200"),
    ("stop_added", "saturating"), ("stop_added", "clamped"), ("compact_row", "four_tiles"),
    ("compact_row", "random_200")])
def test_each_wrong_reference_fails_every_gate(dev, mutation, name):
    case = BY_NAME[name]
    c = 5
    f, v, m, want = ref(name, c)
    wrong = R.walk(case, f, v, m, mutate=mutation)
    got = dict(out=fwd(case, dev, f), grad=grads(case, dev, v, c), q=sums(case, dev, c, m) / Q24)
    assert R.passes(R.gate(want, **got))
    bad = R.gate(wrong, **got)
    assert all(x > 1.0 for x in bad.values()), (mutation, name, bad)


# ---------------------------------------------------------------------------- 7. lifting
W7, H7 = 48, 32
CAMS7 = ((0.0, 0.0, -8.0), (0.15, 0.1, -8.0))


@pytest.fixture(scope="module")
def lift_views(dev, scene):
    """Per view a (Camera, gt, None) device triple and the label map made from the median splat's id: id -> group, no
    median -> 255."""
    import torch

    views, labels = [], []
    with torch.no_grad():
        for pos in CAMS7:
            cam = _camera(W7, H7, pos)
            img, _, _, ids, _ = scene.render_median_depth(cam, (W7, H7))
            lab = torch.where(ids < 0, torch.full_like(ids, 255), (ids >= N_GROUP).to(ids.dtype)).to(torch.uint8)
            views.append((cam, img, None))
            labels.append(lab.contiguous())
    torch.cuda.synchronize()
    return views, labels


def test_lift_labels_recovers_the_groups(dev, scene, lift_views):
    import torch

    from brush_amd import lift_labels, splat_contributions

    views, label_maps = lift_views
    for lab in label_maps:
        vals = set(np.unique(lab.cpu().numpy()).tolist())
        assert vals == {0, 1, 255}, vals
    labels, fs = lift_labels(scene, views, label_maps, 2)
    n = scene.num_splats()
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (n,) and fs.views == 2
    assert tuple(fs.sum.shape) == (n, 2) and tuple(fs.weight.shape) == (n,)
    got = labels.cpu().numpy()
    weight = fs.weight.cpu().numpy()
    group = (np.arange(n) >= N_GROUP).astype(np.int32)
    seen = weight != 0
    assert np.array_equal(got[seen], group[seen])
    assert (got[~seen] == -1).all()
    c = splat_contributions(scene, [(cam, (W7, H7)) for cam, _, _ in views])
    assert int((got == -1).sum()) == int((c.sum == 0).sum()) >= N_OFF
    # the weight is the contribution sum, the class sums never exceed it
    assert np.array_equal(weight, np.rint(c.sum.numpy() * Q24).astype(np.int64))
    s = fs.sum.cpu().numpy()
    assert (s.sum(axis=1) <= weight).all() and (s >= 0).all()
    mean = fs.mean()
    assert mean.dtype == torch.float32 and mean.device == fs.sum.device
    want_mean = np.where(seen[:, None], s / np.maximum(weight, 1)[:, None], 0.0).astype(np.float32)
    assert np.array_equal(mean.cpu().numpy(), want_mean)
    # bitwise repeatable; min_weight takes the faint ones away
    labels2, fs2 = lift_labels(scene, views, label_maps, 2)
    assert torch.equal(labels, labels2) and torch.equal(fs.sum, fs2.sum) and torch.equal(fs.weight, fs2.weight)
    r = fs.read()
    assert r.sum.device.type == "cpu" and torch.equal(r.sum, fs.sum.cpu()) and r.views == 2
    strict, _ = lift_labels(scene, views, label_maps, 2, min_weight=5.0)
    strict = strict.cpu().numpy()
    assert np.array_equal(strict == -1, s.max(axis=1) <= 5.0 * Q24) and (strict == -1).sum() > (got == -1).sum()
    # a mask rules pixels out of both the sums and the weight
    mask = torch.ones((H7, W7), dtype=torch.uint8, device=dev)
    mask[:, :W7 // 2] = 0
    masked = [(cam, img, mask) for cam, img, _ in views]
    _, fm = lift_labels(scene, masked, label_maps, 2)
    assert not bool(fm.sum[:, 0].any()) and bool(fm.sum[:, 1].any()) and bool((fm.weight <= fs.weight).all())
    _, fu = lift_labels(scene, masked, label_maps, 2, use_masks=False)
    assert torch.equal(fu.sum, fs.sum)
    # the cut: Splats.select by label
    right = scene.select(labels == 1)
    assert right.num_splats() == int((got == 1).sum()) and bool((right.means[:, 0] > 0).all())


def test_feature_maps_u8_and_f32_agree_and_render_back(dev, scene, lift_views):
    import torch

    from brush_amd import splat_feature_sums

    views, label_maps = lift_views
    hot = [torch.as_tensor(R.one_hot(l.cpu().numpy(), 3), device=dev) for l in label_maps]
    a = splat_feature_sums(scene, views, hot)
    b = splat_feature_sums(scene, views, [(m * 255).to(torch.uint8) for m in hot])
    c = splat_feature_sums(scene, views, label_maps, num_classes=3)
    assert torch.equal(a.sum, b.sum) and torch.equal(a.sum, c.sum) and torch.equal(a.weight, c.weight)
    assert not bool(a.sum[:, 2].any()) and bool(a.sum[:, :2].any())
    # rendering the lifted means back gives the label image where the scene is opaque
    cam = views[0][0]
    img, feat, _ = scene.render_features(cam, (W7, H7), a.mean())
    lab = label_maps[0].cpu().numpy()
    arg = feat[..., :2].argmax(dim=2).cpu().numpy()
    solid = (img[..., 3] > 0.9).cpu().numpy() & (lab != 255)
    assert solid.sum() > 100 and np.array_equal(arg[solid], lab[solid])


def test_feature_sums_with_resident_views_do_not_synchronise(dev, scene, lift_views):
    import torch

    from brush_amd import splat_feature_sums

    views, label_maps = lift_views
    hot = [torch.as_tensor(R.one_hot(l.cpu().numpy(), 2), device=dev) for l in label_maps]
    splat_feature_sums(scene, views, label_maps, num_classes=2)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.zeros(1, device=dev).item()  # the mode sees a read-back
        a = splat_feature_sums(scene, views, label_maps, num_classes=2)
        b = splat_feature_sums(scene, views, hot)
        means = a.mean(), b.mean()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(a.sum, b.sum) and bool(a.sum.any()) and all(bool(torch.isfinite(m).all()) for m in means)


# ---------------------------------------------------------------------------- 8. refusals
def test_refusals(dev, scene, lift_views):
    import torch

    from brush_amd import features as F

    case = BY_NAME["ragged_17x9"]
    u, aux = _aux(case, dev)
    n, h, w = case["n"], case["h"], case["w"]
    f = torch.zeros((n, 5), device=dev)
    with pytest.raises(ValueError, match="features must be"):
        F.features_from_aux(u, aux, f.double())
    with pytest.raises(ValueError, match="features must be"):
        F.features_from_aux(u, aux, f.cpu())
    with pytest.raises(ValueError, match="features must be"):
        F.features_from_aux(u, aux, f[:, 0])
    with pytest.raises(ValueError, match="features must be"):
        F.features_from_aux(u, aux, f.t())  # not contiguous
    for c in (0, 65):
        with pytest.raises(ValueError, match="channel count"):
            F.features_from_aux(u, aux, torch.zeros((n, c), device=dev))
        with pytest.raises(ValueError, match="channel count"):
            F.feature_grads_from_aux(u, aux, torch.zeros((h, w, c), device=dev), torch.zeros((n, c), device=dev))
        with pytest.raises(ValueError, match="channel count"):
            F.feature_sums_from_aux(u, aux, torch.zeros((h, w, c), device=dev),
                                    torch.zeros((n, c), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        F.features_from_aux(u, aux, f, out=torch.zeros((w, h, 5), device=dev))
    with pytest.raises(ValueError, match="v_out must be"):
        F.feature_grads_from_aux(u, aux, torch.zeros((h, w, 4), device=dev), f)
    with pytest.raises(ValueError, match="v_features must be"):
        F.feature_grads_from_aux(u, aux, torch.zeros((h, w, 5), device=dev), f.to(torch.float64))
    s = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="sums must be"):
        F.feature_sums_from_aux(u, aux, torch.zeros((h, w, 5), device=dev), s.to(torch.int32))
    with pytest.raises(ValueError, match="maps must be"):
        F.feature_sums_from_aux(u, aux, torch.zeros((h, w, 4), device=dev), s)
    with pytest.raises(ValueError, match="label image must be"):
        F.feature_sums_from_aux(u, aux, torch.zeros((w, h), dtype=torch.uint8, device=dev), s)
    with pytest.raises(ValueError, match="maps must be"):
        F.feature_sums_from_aux(u, aux, torch.zeros((h, w, 5)), s)  # on the CPU
    # the ABI itself refuses C = 0 and 65
    from brush_amd import _lib
    import ctypes as C

    st = aux._as_struct()
    for c in (0, 65):
        assert _lib.lib().brush_render_features(C.byref(u), C.byref(st), f.data_ptr(), c, f.data_ptr(), n, None) == -1
    views, label_maps = lift_views
    with pytest.raises(ValueError, match="remap"):
        F.lift_labels(scene, views, label_maps, 65)
    with pytest.raises(ValueError, match="num_classes"):
        F.splat_feature_sums(scene, views, label_maps)
    with pytest.raises(ValueError, match="one map per view"):
        F.splat_feature_sums(scene, views, label_maps[:1], num_classes=2)
    with pytest.raises(ValueError, match="features must be"):
        scene.render_features(views[0][0], (W7, H7), torch.zeros((3, 4), device=dev))
    with pytest.raises(ValueError, match="channel count"):
        scene.render_features(views[0][0], (W7, H7), torch.zeros((scene.num_splats(), 65), device=dev))


# ---------------------------------------------------------------------------- 9. the command line
def test_lift_command_line(dev, tmp_path):
    import json

    import torch
    from PIL import Image

    import brush_amd
    from brush_amd import lift
    from tests import eval_data as E

    rng = np.random.default_rng(23)
    n, w, h = 200, 48, 32
    means = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    sh = rng.uniform(-0.5, 0.5, (n, 1, 3)).astype(np.float32)
    quats = rng.normal(size=(n, 4)).astype(np.float32)
    raw = rng.uniform(1.0, 4.0, n).astype(np.float32)
    log_scales = np.log(rng.uniform(0.08, 0.15, (n, 3))).astype(np.float32)
    src = brush_amd.Splats(*(torch.from_numpy(a).to(dev) for a in (means, sh, quats, raw, log_scales)))
    ply = tmp_path / "cloud.ply"
    ply.write_bytes(src.to_ply())
    E.write_nerf(str(tmp_path / "nerf"), w, h, n_train=2, n_val=1)
    seg = tmp_path / "seg"
    seg.mkdir()
    lab = np.zeros((h, w), np.uint8)
    lab[:, w // 2:] = 1
    lab[:4] = 255
    for i in range(2):
        Image.fromarray(lab, mode="L").save(seg / f"r_{i}.png")
    out = {k: tmp_path / v for k, v in (("labels", "labels.npy"), ("ply", "right.ply"), ("json", "lift.json"),
                                        ("render", "render"))}
    rc = lift.main([str(ply), str(tmp_path / "nerf"), "--labels", str(seg), "--num-classes", "2", "--views", "all",
                    "--export-labels", str(out["labels"]), "--select", "1", "--export", str(out["ply"]),
                    "--render-dir", str(out["render"]), "--json", str(out["json"])])
    assert rc == 0
    got = np.load(out["labels"])
    info = json.loads(out["json"].read_text())
    assert got.shape == (n,) and got.dtype == np.int32 and set(np.unique(got).tolist()) <= {-1, 0, 1}
    assert (got == 0).any() and (got == 1).any()
    assert info["num_views"] == 3 and info["num_classes"] == 2 and info["num_splats"] == n
    assert [c["splats"] for c in info["classes"]] == [int((got == 0).sum()), int((got == 1).sum())]
    assert info["unlabelled"] == int((got < 0).sum()) and all(c["weight"] > 0 for c in info["classes"])
    cut = brush_amd.Splats.from_ply(str(out["ply"]), dev)
    assert cut.num_splats() == int((got == 1).sum())
    pngs = sorted(os.listdir(out["render"]))
    assert len(pngs) == 1 == info["rendered_views"]
    img = np.asarray(Image.open(out["render"] / pngs[0]))
    assert img.shape == (h, w) and img.dtype == np.uint8 and set(np.unique(img).tolist()) <= {0, 1, 255}
    assert (img != 255).any()
    # a view without a label image is refused by name
    (seg / "r_1.png").unlink()
    assert lift.main([str(ply), str(tmp_path / "nerf"), "--labels", str(seg)]) == 2
