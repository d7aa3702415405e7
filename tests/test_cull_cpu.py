"""The cull clouds sit where they claim, and Phase A's bound holds on them with teeth to spare (CPU only).

tests/test_gpu_cull.py compares the GPU's visible set with the oracle's on the clouds of tests/cull_clouds.py.  What
needs no GPU is shown here, against the oracle (oracle.render_forward, which has no prefilter: it runs the exact cull
of project_forward.wgsl on every splat):

  * no oracle-visible splat fails `phase_a_pass`, the f32 restatement of the Phase A prefilter of k_project_cull, on
    any off_frame, near_plane or quat_norm cloud, non-unit quaternions up to |q| = 1.1 included;
  * every off_frame cloud exercises both sides of both decisions: at least 5 % of its splats are rejected by Phase A,
    5 % pass it and fall to the exact cull, 5 % are visible with their centre outside the frame;
  * the clouds have teeth: with cull_k scaled by 1/8 Phase A does reject oracle-visible splats;
  * |q| = 2, outside the documented contract of render_splats, does make Phase A reject oracle-visible splats;
  * the near-plane classes fall on the side of `p_view.z > 0.01f` they name;
  * the compaction builder's visible set is the chosen index set, in ascending order.

Measured (printed by test_teeth_and_margins with -s):

  largest phase_a_margin among oracle-visible splats (Phase A rejects above 1):
      off_frame, 30 clouds         0.554
      off_frame_tight, 5 clouds    0.572   (the bound without its |W|_F^2 = 3 slack would give 1 / sqrt(3.03) = 0.574)
      quat_norm |q| = 0.25 / 1.1   0.425 / 0.603
      quat_norm |q| = 2            2.96    (243 of 4000 splats wrongly rejected: out of contract)
  oracle-visible splats rejected with cull_k scaled by
      1/8    1/6   1/5   1/4   1/3.5  1/3.2  1/3.03  1/3
      777    167   50    10    1      0      0       0      off_frame (114 000 splats)
      2023   796   401   171   65     19     0       0      off_frame_tight (19 000 splats)
  so the smallest scaling that still shows a violation is 1/3.5 on off_frame (the issue's distribution with a quarter
  of the splats sized against Phase A's own bound, see cull_clouds.off_frame) and 1/3.2 on the needles at the clamp
  limit: the tight sub-class reaches the last factor of the derivation, the |W|_F^2 = 3 that an
  orthonormal view rotation never uses up.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import cull_clouds as CC

K_SCALES = (1 / 8, 1 / 6, 1 / 5, 1 / 4, 1 / 3.5, 1 / 3.2, 1 / 3.03, 1 / 3)

_RUNS = {}


def _run(key, build):
    """The case, its uniforms and the oracle's visible mask, once per module."""
    if key not in _RUNS:
        case = build()
        u, c = CC.uniforms(case), case["cloud"]
        n = c["means"].shape[0]
        # the lists are not needed here: a capacity of 1 keeps the oracle from rasterizing whole-frame splats
        _, oa = O.render_forward(u, c["means"], c["log_scales"], c["quats"], c["sh"], c["raw_opac"], max_intersects=1)
        V = int(oa["num_visible"][0])
        vis = np.zeros(n, bool)
        vis[oa["global_from_compact_gid"][:V]] = True
        _RUNS[key] = (case, u, vis, oa["global_from_compact_gid"][:V].copy())
    return _RUNS[key]


def _off_frame(name):
    return _run(("off", name), lambda: CC.off_frame(**CC.OFF_FRAME_CASES[name]))


def _tight(name):
    return _run(("tight", name), lambda: CC.off_frame_tight(**CC.OFF_FRAME_TIGHT_CASES[name]))


def _quat(scale):
    return _run(("quat", scale), lambda: CC.quat_norm(scale))


def _check_phase_a(tag, case, u, vis, shares=True):
    c = case["cloud"]
    n = vis.size
    passed = CC.phase_a_pass(u, c["means"], c["log_scales"])
    wrong = vis & ~passed
    outside = ~CC.centre_in_frame(u, c["means"])
    s_rej, s_exact, s_vis_out = (~passed).mean(), (passed & ~vis).mean(), (vis & outside).mean()
    margin = CC.phase_a_margin(u, c["means"], c["log_scales"])
    print(f"[cull {tag}] n {n} V {int(vis.sum())} | rejected by Phase A {s_rej:.3f}, passed and culled exactly {s_exact:.3f}, "
          f"visible with the centre outside {s_vis_out:.3f} | wrongly rejected {int(wrong.sum())}, largest margin of a "
          f"visible splat {margin[vis].max() if vis.any() else 0.0:.4f}")
    assert not wrong.any(), f"{tag}: Phase A rejects {int(wrong.sum())} splats the oracle keeps"
    if shares:
        assert min(s_rej, s_exact, s_vis_out) >= 0.05, (tag, s_rej, s_exact, s_vis_out)
    return float(margin[vis].max()) if vis.any() else 0.0


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_CASES))
def test_off_frame_no_wrong_rejection_both_sides(name):
    case, u, vis, _ = _off_frame(name)
    assert not CC.centre_in_frame(u, case["cloud"]["means"]).any()  # every centre is off-frame by construction
    _check_phase_a(f"off_frame {name}", case, u, vis)


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_TIGHT_CASES))
def test_off_frame_tight_no_wrong_rejection_both_sides(name):
    case, u, vis, _ = _tight(name)
    c = case["cloud"]
    assert not CC.centre_in_frame(u, c["means"]).any()
    assert CC.clamped_share(u, c["means"]).all()  # t / z on its clamp on some axis, for every splat
    s = np.sort(c["log_scales"].astype(np.float64), axis=1)
    assert (s[:, 2] - s[:, 1] >= np.log(100.0) - 1e-5).all()  # the long axis at least 100 x the others
    _check_phase_a(f"off_frame_tight {name}", case, u, vis)


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_TIGHT_HARD_CASES))
def test_off_frame_tight_hard_no_wrong_rejection(name):
    """The needles of aspect up to 1000 at the wide fields of view: the same cull properties, and alpha at the 1/255
    threshold uncertain by more than 0.03 in f32, which is why the GPU module compares them without pixels."""
    case, u, vis, _ = _run(("hard", name), lambda: CC.off_frame_tight(**CC.OFF_FRAME_TIGHT_HARD_CASES[name]))
    c = case["cloud"]
    assert not CC.centre_in_frame(u, c["means"]).any() and CC.clamped_share(u, c["means"]).all()
    _check_phase_a(f"off_frame_tight hard {name}", case, u, vis)
    _, oa = O.render_forward(u, c["means"], c["log_scales"], c["quats"], c["sh"], c["raw_opac"], max_intersects=4_000_000)
    band = CC.alpha_band_at_threshold(case, oa)
    print(f"[cull off_frame_tight hard {name}] relative f32 uncertainty of alpha at 1/255: max {band.max():.2e}")
    assert band.max() > 0.03


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_TIGHT_CASES))
def test_off_frame_tight_pixels_are_computable(name):
    """The needles are an f32 conditioning hazard for the PIXEL check, not for the cull: a case whose entries at the
    alpha = 1/255 threshold carry a relative f32 uncertainty above 0.03 (1.2e-4 absolute, the pixel tolerance) has
    pixels that two admissible f32 evaluations colour differently.  Every tight case stays below that."""
    case, u, _, _ = _tight(name)
    c = case["cloud"]
    _, oa = O.render_forward(u, c["means"], c["log_scales"], c["quats"], c["sh"], c["raw_opac"], max_intersects=4_000_000)
    band = CC.alpha_band_at_threshold(case, oa)
    print(f"[cull off_frame_tight {name}] entries near alpha = 1/255 on 6000 pixels: {band.size}, relative f32 uncertainty "
          f"median {np.median(band):.2e} max {band.max():.2e}")
    assert band.size > 500 and band.max() <= 0.03


@pytest.mark.parametrize("scale", CC.QUAT_NORMS_IN_CONTRACT)
def test_quat_norm_in_contract(scale):
    """|q| = 0.25 and 1.1: R(q) = (1 - s^2) I + s^2 R(q / s) has norm |2 s^2 - 1|, which the |W|_F^2 = 3 slack of
    cull_k covers while (2 s^2 - 1)^2 <= 3.03, i.e. up to s = 1.17."""
    case, u, vis, _ = _quat(scale)
    nrm = np.linalg.norm(case["cloud"]["quats"].astype(np.float64), axis=1)
    assert np.allclose(nrm, scale, rtol=1e-6)
    _check_phase_a(f"quat_norm |q|={scale}", case, u, vis)


def test_quat_norm_out_of_contract():
    """|q| = 2: the documented contract (render_splats, brush_hip.h) is not an idle one.  Phase A rejects splats that
    the oracle, and the reference shader, keep."""
    scale = CC.QUAT_NORM_OUT_OF_CONTRACT
    case, u, vis, _ = _quat(scale)
    c = case["cloud"]
    wrong = vis & ~CC.phase_a_pass(u, c["means"], c["log_scales"])
    margin = CC.phase_a_margin(u, c["means"], c["log_scales"])
    print(f"[cull quat_norm |q|={scale}] V {int(vis.sum())}, wrongly rejected {int(wrong.sum())} of {vis.size}, largest margin "
          f"of a visible splat {margin[vis].max():.3f}")
    assert wrong.sum() >= 10 and margin[vis].max() > 1.0


def test_teeth_and_margins():
    """cull_k scaled by 1/8: the off-frame set as a whole yields oracle-visible splats that Phase A rejects.  Prints the
    violations at every scaling of K_SCALES and the largest margin of a visible splat (the module docstring's
    figures)."""
    for label, cases, get in (("off_frame", CC.OFF_FRAME_CASES, _off_frame), ("off_frame_tight", CC.OFF_FRAME_TIGHT_CASES, _tight)):
        viol = {k: 0 for k in K_SCALES}
        worst, total = 0.0, 0
        for name in cases:
            case, u, vis, _ = get(name)
            c = case["cloud"]
            total += vis.size
            worst = max(worst, float(CC.phase_a_margin(u, c["means"], c["log_scales"])[vis].max()))
            e = CC.exp_max_log_scale(c["log_scales"])
            for k in K_SCALES:
                viol[k] += int((vis & ~CC.phase_a_pass(u, c["means"], c["log_scales"], k_scale=k, exp_smax=e)).sum())
        with_viol = [k for k in K_SCALES if viol[k]]
        print(f"[cull teeth {label}] {total} splats, largest margin of a visible splat {worst:.4f}; violations by cull_k "
              f"scaling: " + ", ".join(f"1/{1 / k:.3g}: {v}" for k, v in viol.items())
              + f"; smallest scaling with violations: 1/{1 / max(with_viol):.3g}")
        assert viol[1 / 8] >= 1
        assert worst < 1.0
    assert viol[1 / 4] >= 1  # the tight sub-class bites well below the issue's 1/6


def test_near_plane_classes():
    """nextafter(0.01f, 0) and 0.01f itself are culled, wherever the centre is; nextafter(0.01f, 1), 0.0100001f and 0.02f
    are kept whenever the centre is in the frame (the 0.3 px^2 blur alone gives a radius of 2 px)."""
    case, u, vis, _ = _run("near", CC.near_plane)
    c = case["cloud"]
    assert np.array_equal(np.unique(c["means"][:, 2]), np.sort(CC.NEAR_DEPTHS))
    inside = CC.centre_in_frame(u, c["means"])
    for k, keep in enumerate(CC.NEAR_DEPTHS_VISIBLE):
        m = case["depth_class"] == k
        print(f"[cull near_plane] z = {float(CC.NEAR_DEPTHS[k])!r}: {int(m.sum())} splats, {int((m & inside).sum())} in frame, "
              f"{int((m & vis).sum())} visible")
        assert (m & inside).sum() >= 50 and (m & ~inside).sum() >= 50
        if keep:
            assert vis[m & inside].all()
            assert not vis[m & ~inside].all()  # tiny splats far outside are culled by the bbox, not the plane
        else:
            assert not vis[m].any()
    _check_phase_a("near_plane", case, u, vis, shares=False)


@pytest.mark.parametrize("kind", CC.EXTREME_CLASSES)
def test_extreme_scale_classes(kind):
    """The oracle survives every class; `huge` and `needle` do produce non-finite records (what nan_equal is for)."""
    case, u, vis, gids = _run(("extreme", kind), lambda: CC.extreme_scale(kind))
    c = case["cloud"]
    ls = c["log_scales"]
    if kind == "huge":
        assert ls.min() >= 20 and ls.max() <= 44
    elif kind == "tiny":
        assert ls.min() >= -104 and ls.max() <= -80
    else:
        assert ((ls >= 20) & (ls <= 44)).sum(axis=1).min() == 1 and ((ls == -90).sum(axis=1) == 2).all()
    _, oa = O.render_forward(u, c["means"], c["log_scales"], c["quats"], c["sh"], c["raw_opac"], max_intersects=200_000)
    V = int(oa["num_visible"][0])
    nonfinite = int((~np.isfinite(oa["projected_splats"][:V])).any(axis=1).sum())
    print(f"[cull extreme_scale {kind}] V {V} of {vis.size}, I {int(oa['num_intersections'][0])}, records with a non-finite "
          f"word {nonfinite}")
    assert 0 < V < vis.size and not oa["overflow"]
    BK.assert_binning_properties(BK.oracle_arrays(oa))  # the property check itself copes with non-finite records
    assert (nonfinite > 0) == (kind != "tiny")


def _check_compaction(pattern, n):
    case, u, vis, gids = _run(("compaction", pattern, n), lambda: CC.compaction(pattern, n))
    chosen = case["chosen"]
    assert chosen.dtype == np.int64 and (np.diff(chosen) > 0).all() and (chosen.size == 0 or (0 <= chosen[0] and chosen[-1] < n))
    assert gids.size == chosen.size, (pattern, n, gids.size, chosen.size)
    assert np.array_equal(gids.astype(np.int64), chosen), (pattern, n)
    _RUNS.pop(("compaction", pattern, n))
    return chosen.size


@pytest.mark.parametrize("n", CC.COMPACTION_SMALL_N)
def test_compaction_builder_small(n):
    """num_visible and global_from_compact_gid of the oracle are the chosen set, ascending, for every pattern."""
    sizes = {p: _check_compaction(p, n) for p in CC.COMPACTION_PATTERNS}
    print(f"[cull compaction n={n}] chosen: {sizes}")
    assert sizes["none"] == 0 and sizes["all"] == n and sizes["first"] == sizes["last"] == 1
    assert sizes["one_per_block"] == -(-n // CC.CULL_BLOCK)


@pytest.mark.parametrize("n", CC.COMPACTION_LARGE_N)
def test_compaction_builder_large(n):
    """The sparse block-boundary pattern on either side of the self-scan switch and at two and four scan chunks."""
    blocks = -(-n // CC.CULL_BLOCK)
    k = _check_compaction(CC.COMPACTION_LARGE_PATTERN, n)
    print(f"[cull compaction n={n}] {blocks} cull workgroups, {-(-blocks // 1024)} scan chunks, chosen {k}")
    assert (blocks <= CC.SELF_SCAN_BLOCKS) == (n == CC.SELF_SCAN_BLOCKS * CC.CULL_BLOCK)
    assert k == 2 * (n // CC.CULL_BLOCK) + (1 if n % CC.CULL_BLOCK else 0)


def test_gradient_case_is_clamped():
    """The gradient leg's cloud: at least half of the oracle-visible splats have t = z * clamp(x / z) on its clamp on
    some axis (calc_cov2d and its derivative in project_bwd.hip), and no pixel sigma exceeds the cap."""
    case, u, vis, _ = _run("grad", lambda: CC.off_frame(**CC.GRAD_CASE))
    c = case["cloud"]
    clamped = CC.clamped_share(u, c["means"])
    share = float(clamped[vis].mean())
    print(f"[cull grad case] V {int(vis.sum())} of {vis.size}, clamped among the visible {share:.3f}")
    assert vis.sum() >= 500 and share >= 0.5
    assert c["raw_opac"].min() >= -2.0 and c["raw_opac"].max() <= 3.0
