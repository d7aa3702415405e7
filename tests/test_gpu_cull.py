"""The projection cull and the compaction at their decision edges (pytest -m gpu).

k_project_cull (project.hip) decides per splat whether it exists for the rest of the frame: a wrong "no" takes the
splat out of the image and out of every gradient, and nothing downstream can notice.  Each case here is a small
directed cloud of tests/cull_clouds.py placed on one kind of decision edge; it runs the GPU forward in both
accumulation modes and the CPU oracle once (the oracle has no prefilter: it applies the exact cull of
project_forward.wgsl to every splat) and asserts

  * the integer state bit-exact against the oracle (tests/binning_check.py): V, I, both gid maps, the projected records
    bitwise, cum_tiles_hit, the tile lists and the bins;
  * the oracle-free properties of the lists (assert_binning_properties);
  * the pixels with _assert_forward_parity(rounding_flips=True), unchanged, on every class with finite records;
  * for the compaction cases, global_from_compact_gid[:V] against the chosen index set itself and
    compact_from_global_gid as its inverse, 0xFFFFFFFF elsewhere, with the buffers poisoned beforehand.

tests/test_cull_cpu.py shows without a GPU that the clouds sit where they claim and that the Phase A restatement has
teeth on them down to cull_k / 3.2.

| decision                                      | cases                                                            |
|-----------------------------------------------|------------------------------------------------------------------|
| Phase A screen bounds vs the exact tile bbox  | off_frame (5 frames x 3 principal points x 2 cameras, both focal |
|                                               | settings), off_frame_tight(_hard): needles on the clamp of t / z |
| Phase A with non-unit quaternions, |q| <= 1.1 | quat_norm 0.25, 1.1                                              |
| p_view.z > 0.01f                              | near_plane (the two f32 neighbours of 0.01f, 0.0100001f, 0.02f)  |
| det == 0, radius, bbox and walk rectangle on  | extreme_scale huge / tiny / needle (records compared nan_equal)  |
| non-finite and saturating values              |                                                                  |
| ballots, rounds, block offsets, self scan     | compaction n = 1 .. 4097 x 8 visibility patterns                 |
| k_compact<true> vs k_cull_scan + <false>      | compaction n = 2048 * 1024, + 1; 2049 * 1024 + 1, 3073 * 1024 + 1|
| t = z * clamp(x / z) and its derivative       | gradients, clamped off-frame cloud (project_bwd.hip)             |

Measured on one MI355X (both modes agree with the oracle in every case; seconds are the whole test, oracle included):

| case                                         |    n |           V |                 I | s          |
|----------------------------------------------|------|-------------|-------------------|------------|
| off_frame 16x16 (6 cases)                    | 4000 | 1696 - 1942 |         556 - 693 | 0.01, 0.35 the first |
| off_frame 100x37 (6)                         | 4000 | 1307 - 1643 |     1 335 - 2 067 | 0.01 - 0.03 |
| off_frame 640x480 (6)                        | 4000 | 1872 - 2202 | 114 655 - 203 644 | 0.09 - 0.20 |
| off_frame 1920x1080 (6)                      | 3000 | 1186 - 1436 | 272 434 - 436 433 | 0.34 - 0.41 |
| off_frame 33x1000 (6)                        | 4000 | 2485 - 2785 |   25 347 - 35 884 | 0.01 - 0.04 |
| off_frame_tight 16x16_c0_rotated_eq          | 4000 |        1774 |               692 | 0.01       |
| off_frame_tight 100x37_c2_identity_uneq      | 4000 |        1868 |               663 | 0.01       |
| off_frame_tight 640x480_c1_rotated_uneq      | 4000 |        1497 |             9 075 | 0.04       |
| off_frame_tight 1920x1080_c0_identity_eq     | 3000 |        1128 |            30 507 | 0.29       |
| off_frame_tight 33x1000_c1_rotated_uneq      | 4000 |        1697 |             6 171 | 0.02       |
| off_frame_tight_hard 640x480_c2 (no pixels)  | 4000 |        1484 |               980 | 0.01       |
| off_frame_tight_hard 640x480_c1 (no pixels)  | 4000 |        1528 |             5 544 | 0.01       |
| off_frame_tight_hard 1920x1080_c0 (no pixels)| 3000 |        1101 |            15 823 | 0.06       |
| quat_norm 0.25 / 1.1                         | 4000 | 1480 / 1789 |  87 774 / 135 922 | 0.07 / 0.09 |
| near_plane                                   | 3000 |         522 |               722 | < 0.01     |
| extreme_scale huge / tiny / needle           | 1500 | 352 / 440 / 418 | 352 / 553 / 2 327 | < 0.01 |
| compaction n = 1 .. 4097, 8 patterns each    | 1 .. 4097 | 0 .. 4097 |      0 .. 11 240 | <= 0.01 each |
| compaction block_edges n = 2 097 152         |      |        4096 |            11 191 | 0.06       |
| compaction block_edges n = 2 097 153         |      |        4097 |            11 240 | 0.05       |
| compaction block_edges n = 2 098 177         |      |        4099 |            11 237 | 0.06       |
| compaction block_edges n = 3 146 753         |      |        6147 |            16 807 | 0.10       |
| gradients with clamped t                     | 2000 |        1406 |             2 457 | 1.05       |

Findings of the first run.  (1) extreme_scale needle: one splat with a finite record (conic 7.6e-20, 4.2e-17, 2.4e-14,
opacity 0.17: it covers the whole frame) got 0 tiles on the GPU and 24 in the oracle.  walk_rect (splat_math.hpp) added
its one tile of slack, - 1 and + 2, AFTER the saturating float-to-int conversion; with a reach of 7e10 px the conversion
gives INT_MIN / INT_MAX, the additions wrapped around and the clamps to the bbox emptied the rectangle.  The slack is
now added in float before the conversion (identical below 2^24 tiles, clamped to the bbox above); k_project_visible,
k_walk_count and k_map_intersects are the three kernels whose code changed.  (2) With needle aspects up to 1000 the
integer state was exact but ~100 pixels per large frame missed the pixel check: alpha at the 1/255 threshold is
uncertain by 0.1 .. 0.9 relative in f32 there.  Those clouds stay as off_frame_tight_hard, compared without pixels; the
off_frame_tight cases keep the uncertainty below 0.03 (asserted in tests/test_cull_cpu.py) and pass the pixel check
unchanged.  Every other edge held at the first run: Phase A, the near plane, the compaction at every seam and scan
shape, |q| = 0.25 and 1.1, and the gradient gate on the clamped branch.
"""
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import cull_clouds as CC
from tests import test_gpu_render as RT

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True
    return torch.device("cuda:0")


def _camera(case):
    import brush_amd

    c = case["camera"]
    return brush_amd.Camera(c["position"], c["rotation_xyzw"], c["fov_x"], c["fov_y"], c["center_uv"])


def _run_case(dev, tag, case, cap, pixels=True, nan_equal=False):
    """Both modes on the GPU, the oracle once (on the uniform words the GPU used), every check.  Returns (the last
    run's numpy aux, V, I, oracle aux)."""
    import torch

    from brush_amd import render as R

    t0 = time.perf_counter()
    (w, h), cloud = case["frame"], case["cloud"]
    n = cloud["means"].shape[0]
    p = {k: RT._t(v, dev) for k, v in cloud.items()}
    runs = []
    for det in (False, True):
        out, aux, _ = R._forward_impl(_camera(case), (w, h), p["means"], p["log_scales"], p["quats"], p["sh"],
                                      p["raw_opac"], False, cap, deterministic=det, expect_backward=False)
        assert aux.deterministic == det and aux.max_intersects == cap
        runs.append((out, aux, R.uniforms_to_numpy(aux)))
    torch.cuda.synchronize()
    u = runs[0][2]
    o_out, o_aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                    cloud["raw_opac"], max_intersects=cap)
    assert not o_aux["overflow"]
    orc = dict(out=o_out, aux=o_aux)
    checked = None
    for out, aux, u_run in runs:
        got = BK.aux_arrays(aux, u_run["num_visible"])
        V, I = BK.assert_integer_parity(got, o_aux, nan_equal=nan_equal)
        BK.assert_binning_properties(got)
        if not pixels or (checked is not None and torch.equal(out, checked[0]) and torch.equal(aux.final_index, checked[1])):
            continue  # no finite image to compare, or the same image and final_index to the bit as the other mode
        RT._assert_forward_parity(dict(out=out.cpu().numpy(), aux=aux, u=u_run), orc, w, h, rounding_flips=True)
        checked = (out, aux.final_index)
    print(f"[cull {tag}] n {n} V {V} I {I} | {time.perf_counter() - t0:.2f} s")
    return got, V, I, o_aux


def _visible_mask(oa, n):
    V = int(oa["num_visible"][0])
    vis = np.zeros(n, bool)
    vis[oa["global_from_compact_gid"][:V]] = True
    return vis


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_CASES))
def test_off_frame(dev, name):
    """Centres 1 .. 5e4 px outside the frame, extents on either side of reaching in: the visible set is the oracle's, and
    a good share of it is there although Phase A's cheap test had the centre far outside."""
    case = CC.off_frame(**CC.OFF_FRAME_CASES[name])
    got, V, I, oa = _run_case(dev, f"off_frame {name}", case, 4_000_000)
    n = case["cloud"]["means"].shape[0]
    assert 0.05 * n <= V <= 0.95 * n and I > 0


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_TIGHT_CASES))
def test_off_frame_tight(dev, name):
    """Needles along the direction that uses up Phase A's bound, centres on or past the clamp limit of t / z."""
    case = CC.off_frame_tight(**CC.OFF_FRAME_TIGHT_CASES[name])
    got, V, I, oa = _run_case(dev, f"off_frame_tight {name}", case, 4_000_000)
    n = case["cloud"]["means"].shape[0]
    assert 0.05 * n <= V <= 0.95 * n and I > 0


@pytest.mark.parametrize("name", list(CC.OFF_FRAME_TIGHT_HARD_CASES))
def test_off_frame_tight_hard(dev, name):
    """The same needles at aspects up to 1000 and wide fields of view.  Integer state and list properties only: alpha at
    the 1/255 threshold is uncertain by 0.1 .. 0.9 in f32 there (tests/test_cull_cpu.py), so two admissible evaluations
    colour some pixels differently, while the cull's decisions do not depend on the aspect."""
    case = CC.off_frame_tight(**CC.OFF_FRAME_TIGHT_HARD_CASES[name])
    got, V, I, oa = _run_case(dev, f"off_frame_tight_hard {name}", case, 4_000_000, pixels=False)
    n = case["cloud"]["means"].shape[0]
    assert 0.05 * n <= V <= 0.95 * n and I > 0


@pytest.mark.parametrize("scale", CC.QUAT_NORMS_IN_CONTRACT)
def test_quat_norm_in_contract(dev, scale):
    """|q| = 0.25 and 1.1, inside the documented contract of render_splats: results equal the reference's."""
    case = CC.quat_norm(scale)
    got, V, I, oa = _run_case(dev, f"quat_norm {scale}", case, 4_000_000)
    assert V > 1000 and I > V


def test_near_plane(dev):
    """p_view.z on nextafter(0.01f, 0), 0.01f, nextafter(0.01f, 1), 0.0100001f and 0.02f: the first two are culled, the
    others are kept wherever the centre is in the frame."""
    case = CC.near_plane()
    got, V, I, oa = _run_case(dev, "near_plane", case, 200_000)
    n = case["cloud"]["means"].shape[0]
    vis = np.zeros(n, bool)
    vis[got["global_from_compact_gid"][:V]] = True
    inside = CC.centre_in_frame(CC.uniforms(case), case["cloud"]["means"])
    for k, keep in enumerate(CC.NEAR_DEPTHS_VISIBLE):
        m = case["depth_class"] == k
        if keep:
            assert vis[m & inside].all()
        else:
            assert not vis[m].any()
    assert V > 400


@pytest.mark.parametrize("kind", CC.EXTREME_CLASSES)
def test_extreme_scale(dev, kind):
    """Covariances that overflow (log-scales 20 .. 44), vanish (-104 .. -80) or do both (needles): the cull's det == 0
    test, the saturating radius and the truncating bbox see inf and NaN.  The records hold NaN where the oracle's do and
    are bitwise equal elsewhere; no pixel check, the image is not finite."""
    case = CC.extreme_scale(kind)
    got, V, I, oa = _run_case(dev, f"extreme_scale {kind}", case, 2_000_000, pixels=False, nan_equal=True)
    n = case["cloud"]["means"].shape[0]
    assert 0 < V < n and I >= V // 2 and not got["overflow"]
    nonfinite = (~np.isfinite(got["projected_splats"][:V])).any(axis=1).sum()
    assert (nonfinite > 0) == (kind != "tiny")


def _check_compaction(dev, pattern, n, pixels):
    case = CC.compaction(pattern, n)
    chosen = case["chosen"]
    got, V, I, oa = _run_case(dev, f"compaction {pattern} n={n}", case, 200_000, pixels=pixels)
    assert V == chosen.size
    assert np.array_equal(got["global_from_compact_gid"][:V].astype(np.int64), chosen), (pattern, n)
    inv = np.full(n, INVALID, np.uint32)
    inv[chosen] = np.arange(V, dtype=np.uint32)
    assert np.array_equal(got["compact_from_global_gid"][:n], inv), (pattern, n)
    assert (I > 0) == (V > 0)
    return V


@pytest.mark.parametrize("n", CC.COMPACTION_SMALL_N)
def test_compaction_small(dev, n):
    """Only index 0, only index n - 1, none, all, the first and last lane of every wave, the first and last splat of every
    256-splat round and of every 1024-splat block, one splat per block: around 64, 256, 1024 and 4096 splats."""
    for pattern in CC.COMPACTION_PATTERNS:
        _check_compaction(dev, pattern, n, pixels=True)


@pytest.mark.parametrize("n", CC.COMPACTION_LARGE_N)
def test_compaction_large(dev, n):
    """2048 cull workgroups (the last size k_compact scans by itself), 2049 and 2050 (k_cull_scan: two full
    chunks of 1024 counts and a third holding one or two) and 3074 (three full chunks and a fourth): two visible splats per workgroup, at its two ends."""
    V = _check_compaction(dev, CC.COMPACTION_LARGE_PATTERN, n, pixels=False)
    assert V >= 2 * CC.SELF_SCAN_BLOCKS


def test_gradients_with_clamped_t(dev):
    """About 1400 visible splats whose centres lie 24 .. 45 px outside a 200x120 frame on the rotated off-centre camera:
    for most of them t = z * clamp(x / z) of calc_cov2d sits on its clamp, so J's third column and its derivative in
    project_bwd.hip take the clamped branch.  Forward parity, then the gradient gate, unchanged."""
    case = CC.off_frame(**CC.GRAD_CASE)
    (w, h), cloud = case["frame"], case["cloud"]
    # on the CPU, before anything runs on the GPU: the case is what it says
    u_cpu = CC.uniforms(case)
    _, oa_cpu = O.render_forward(u_cpu, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                 cloud["raw_opac"], max_intersects=1)
    vis = _visible_mask(oa_cpu, cloud["means"].shape[0])
    share = float(CC.clamped_share(u_cpu, cloud["means"])[vis].mean())
    print(f"[cull gradients] visible {int(vis.sum())}, clamped among them {share:.3f}")
    assert vis.sum() >= 500 and share >= 0.5
    t0 = time.perf_counter()
    gpu, orc = RT._run_pair(dev, cloud, w, h, 0, max_intersects=200_000, camera=_camera(case))
    V, I = RT._assert_forward_parity(gpu, orc, w, h, rounding_flips=True)
    assert V >= 500 and I > V
    BK.assert_binning_properties(BK.aux_arrays(gpu["aux"], gpu["u"]["num_visible"]))
    RT._assert_grad_parity(gpu, orc, "cull_clamped")
    print(f"[cull gradients] n {cloud['means'].shape[0]} V {V} I {I} | {time.perf_counter() - t0:.2f} s")
