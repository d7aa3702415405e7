"""Tile binning at every regime switch, on small directed clouds (pytest -m gpu).

The tile-binning middle of the forward (tile_count.hip, tile_emit.hip, tile_walk.hpp, the tile sort) chooses its code
paths at run time from device-side counts.  Each case here builds a cloud for ONE of those switches
(tests/binning_clouds.py), runs the GPU forward in both accumulation modes (deterministic: the permutation-carrying
sort and k_tile_bin_edges; default: the edges out of the sort's last pass) and the CPU oracle once, and asserts

  * the integer state bit-exact against the oracle (tests/binning_check.py, shared with test_gpu_render.py);
  * the pixels, with _assert_forward_parity's own check and tolerance (see the note on rounding flips below);
  * properties of the lists that need no oracle (bins partition [0, I) in tile order, gids ascend inside a bin,
    entries per splat = steps of cum_tiles_hit, every entry inside its splat's bbox);
  * that the case sits in the regime it names: V from aux (exact by construction), classes and queue items from
    binning_clouds.classify, at least 20 % away from every item-count threshold.

| switch                                   | cases                                                          |
|------------------------------------------|----------------------------------------------------------------|
| V vs 2^18 (32 / 64 splats per wave)      | v_262144, v_262145                                             |
| V > 2^19 (inline up to 16 / 64 tiles)    | v_524288, v_524289                                             |
| V >= 2^19 (flattened inline emission)    | v_524287, v_524288 (with the 16-tile limit), flat_truncated    |
| queue items: 4 / 16 / 64 per wave        | group16, group64, group64_1080p                                |
| queue items vs capacity N                | group64_queue_overflow, unknown_inline_retest                  |
| reach unknown (det Q * 1024 < q0 q2)     | unknown_queued, unknown_inline_retest                          |
| tile-count bits <= 8, <= 16, > 16        | tiles_*, wide_* (both sort shapes above 65 535 tiles)          |

Measured on one MI355X (both modes agree to the bit in every case; seconds are the whole test, oracle included):

| case                    |      V |          I | small / mid / big (classify) | items / capacity  | s    |
|-------------------------|--------|------------|------------------------------|-------------------|------|
| v_262144                | 262144 |  1 246 077 | 254 178 / 4 755 / 3 211      | 13 093 / 263 144  | 0.96 |
| v_262145                | 262145 |  1 244 769 | 254 186 / 4 756 / 3 203      | 13 031 / 263 145  | 0.40 |
| v_524287                | 524287 |  2 497 920 | 508 211 / 9 686 / 6 390      | 26 339 / 525 287  | 0.69 |
| v_524288                | 524288 |  2 498 586 | 508 225 / 9 592 / 6 471      | 26 365 / 525 288  | 0.73 |
| v_524289                | 524289 |  2 501 768 | 508 222 / 9 647 / 6 420      | 16 802 / 525 289  | 0.88 |
| flat_truncated          | 524289 |  1 000 003 | (the v_524289 cloud; 2 501 768 hits, overflow)  | | 0.38 |
| group16                 | 100000 |  3 407 778 | 60 031 / 11 629 / 28 340     | 92 104 / 100 000  | 0.37 |
| group64                 | 400000 |  8 520 119 | 240 329 / 49 506 / 110 165   | 326 941 / 400 000 | 0.89 |
| group64_1080p           | 400000 |  8 343 729 | 240 351 / 48 633 / 111 016   | 322 600 / 400 000 | 1.14 |
| group64_queue_overflow  | 300000 | 14 773 945 | 74 888 / 52 055 / 173 057    | 513 806 / 300 000 | 1.33 |
| unknown_queued          |  20000 |    826 631 | 0 / 79 / 19 921 (12 490 of unknown reach) | 199 709 / 220 000 | 0.59 |
| unknown_inline_retest   |  20000 |    828 486 | 0 / 89 / 19 911 (12 477 of unknown reach) | 199 242 / 20 000  | 0.58 |
| tiles_1 .. tiles_256    |  60000 | 57 640 .. 650 997 | all small up to 16 tiles; 49 871 / 6 791 / 3 338 at 256 | <= 14 481 / 60 000 | < 0.1 |
| tiles_4095, tiles_4096  |  60000 | 804 759, 808 238 | 49 856 / 5 336 / 4 808 | 18 417 / 60 000   | 0.22 |
| wide_65535 .. 65792     |  60000 | 857 169 .. 857 727 | 49 852 / 4 912 / 5 236 | 19 877 / 60 000   | 1.9  |
| wide_65552 (4097 x 16)  |  60000 |    689 229 | 50 015 / 6 184 / 3 801       | 15 458 / 60 000   | 1.9  |
| gradients, 65 792 tiles |  60000 |    857 727 |                              |                   | 5.4  |

In v_524289 the items (16 802) sit 3 % above the 4 / 16 switch of walk_group: that case names V only, and which group
size it takes is not asserted.  In group64_queue_overflow and unknown_inline_retest the consumers see
min(items, capacity) = N, exact by construction.

Every integer output and every property held at the first run, above 65 535 tiles included.  The pixel check did not,
and not because of the kernels: with thin tilted splats at opacity 0.9-0.99 a handful of pixels per frame (1-11; ~650 of
2^20 with the aspect-300 splats) have an entry whose `alpha >= 1/255` test, or a stop test, is decided by the f32
rounding of sigma's cancelling terms, far outside the oracle's 1e-5 guard band; the GPU (fused multiply-adds) and the
oracle (none) then take different, equally admissible decisions.  These cases therefore run the pixel check with
rounding_flips=True (tests/test_gpu_render.py: _rounding_flip_explains): such a pixel must equal the f64 composite under
one of the at most 16 decision sets that rounding allows, to the unchanged tolerance and with the same final_index;
tests/test_binning_cpu.py shows that a pixel off by 5e-4 or by one entry is not excused.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import binning_check as BK
from tests import binning_clouds as BC
from tests import test_gpu_render as RT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import brush_amd.render as R

    R.DEBUG_POISON = True
    return torch.device("cuda:0")


_CLOUD = {}   # one slot each: consecutive cases share a cloud (flat_truncated, the two caps of a wide frame)
_ORACLE = {}


def _cloud(name):
    c = BC.CASES[name]
    key = repr((sorted(c["cloud"].items()), c["w"], c["h"]))
    if key not in _CLOUD:
        _CLOUD.clear()
        _CLOUD[key] = BC.case_cloud(name)
    return key, _CLOUD[key]


def _oracle(key, cloud, u, cap):
    """The oracle's forward for this cloud and frame.  A run that did not overflow serves every capacity that holds
    its list: the oracle's outputs do not depend on the capacity then."""
    hit = _ORACLE.get(key)
    if hit is not None and not hit[1]["overflow"] and int(hit[1]["num_intersections"][0]) <= cap \
            and all(np.array_equal(np.asarray(hit[2][k]), np.asarray(u[k])) for k in hit[2]):
        return hit[0], hit[1]
    _ORACLE.clear()
    o_out, o_aux = O.render_forward(u, cloud["means"], cloud["log_scales"], cloud["quats"], cloud["sh"],
                                    cloud["raw_opac"], max_intersects=cap)
    _ORACLE[key] = (o_out, o_aux, {k: u[k] for k in ("viewmat", "focal", "img_size", "tile_bounds", "pixel_center")})
    return o_out, o_aux


def _run_case(dev, name):
    """Both modes on the GPU, the oracle once, every check but the regime.  Returns (regime dict, V, I, oracle aux)."""
    import torch

    from brush_amd import render as R

    c = BC.CASES[name]
    w, h, cap = c["w"], c["h"], c["cap"]
    key, cloud = _cloud(name)
    n = cloud["means"].shape[0]
    p = {k: RT._t(v, dev) for k, v in cloud.items()}
    runs = []
    for det in (False, True):
        out, aux, _ = R._forward_impl(RT._camera(w, h), (w, h), p["means"], p["log_scales"], p["quats"], p["sh"],
                                      p["raw_opac"], False, cap, deterministic=det, expect_backward=False)
        assert aux.deterministic == det and aux.max_intersects == cap
        runs.append((det, out, aux, R.uniforms_to_numpy(aux)))
    torch.cuda.synchronize()
    u = runs[0][3]
    o_out, o_aux = _oracle(key, cloud, u, cap)
    orc = dict(out=o_out, aux=o_aux)
    checked = None
    for det, out, aux, u_run in runs:
        got = BK.aux_arrays(aux, u_run["num_visible"])
        V, I = BK.assert_integer_parity(got, o_aux)
        BK.assert_binning_properties(got)
        if checked is not None and torch.equal(out, checked[0]) and torch.equal(aux.final_index, checked[1]):
            continue  # the same image and final_index to the bit: the pixel check would repeat itself
        RT._assert_pixel_parity(dict(out=out.cpu().numpy(), aux=aux, u=u_run), orc, rounding_flips=True)
        checked = (out, aux.final_index)
    r = BC.regime(got["projected_splats"][:V], u["tile_bounds"], n)
    r.update(I=I, overflow=got["overflow"], num_tiles=int(u["tile_bounds"][0]) * int(u["tile_bounds"][1]))
    print(f"[binning {name}] n {n} V {V} I {I} overflow {got['overflow']} tiles {r['num_tiles']} | small/mid/big "
          f"{r['n_small']}/{r['n_mid']}/{r['n_big']} (no tile: {r['n_zero']}, reach unknown: {r['n_unknown']}) | inline limit "
          f"{r['inline_limit']}, queued splats {r['n_queued']}, items {r['items']} of capacity {r['capacity']}")
    return r, V, I, o_aux


@pytest.mark.parametrize("V", BC.V_BOUNDARIES)
def test_visible_count_boundaries(dev, V):
    """V on either side of kHalfWaveSplats (a wave takes 32 or 64 splats), of kSmallAreaSwitch (inline walks of up to 16
    or 64 tiles) and of kFlatEmitMin (lane-private or wave-flattened inline emission); V = 2^19 exactly is the one
    combination of flattened emission with the 16-tile limit.  1 000 hidden splats are interleaved, so compaction
    runs and the queue capacity N exceeds V."""
    r, v, I, _ = _run_case(dev, f"v_{V}")
    assert v == V == r["V"] and r["capacity"] == V + 1000
    assert r["half_wave"] == (V <= 1 << 18) and r["flat_emit"] == (V >= 1 << 19)
    assert r["inline_limit"] == (64 if V > 1 << 19 else 16)
    assert min(r["n_small"], r["n_mid"], r["n_big"]) > 1000, r  # every inline / queued class is there
    assert r["n_zero"] > 1000  # visible, no tile (opacity below 1/255)
    assert 0 < r["items"] <= r["capacity"] and not r["overflow"]


def test_flat_emission_truncated(dev):
    """The wave-flattened emission (V > 2^19) with a list cut at a capacity that is no multiple of anything: the
    overflow is flagged, I is the capacity and the list is the oracle's truncated list."""
    r, V, I, oa = _run_case(dev, "flat_truncated")
    assert V == (1 << 19) + 1 and r["flat_emit"] and r["inline_limit"] == 64
    assert r["overflow"] == 1 and I == 1_000_003 == BC.CASES["flat_truncated"]["cap"]
    assert int(oa["cum_tiles_hit"][-1]) > 2 * I  # more than half of the entries fall off the end


def test_walk_group_16(dev):
    """Between 16 384 and 2^18 queue items: 16 per consumer wave."""
    r, V, I, _ = _run_case(dev, "group16")
    assert 1.2 * BC.GROUP4_MAX < r["items"] < 0.8 * BC.GROUP16_MAX and r["items"] <= r["capacity"], r
    assert r["group"] == 16 and not r["overflow"]


@pytest.mark.parametrize("name", ["group64", "group64_1080p"])
def test_walk_group_64(dev, name):
    """More than 2^18 queue items: 64 per consumer wave, the cross-group `before` sum of the emit pass over thousands of
    groups; 8.5 M intersections in a 12 M buffer (the 3-launch sort shape).  Once more on 1920x1080: ragged tile rows."""
    r, V, I, _ = _run_case(dev, name)
    assert r["items"] > 1.2 * BC.GROUP16_MAX and r["items"] <= r["capacity"], r
    assert r["group"] == 64 and not r["overflow"] and I > 8_000_000


def test_walk_group_64_queue_overflow(dev):
    """More items than the queue holds (capacity = N = 300 000 > 2^18, so the consumers still take 64 per wave): the
    splats past the end are walked inline by both passes, one reservation leaves sentinel holes."""
    r, V, I, _ = _run_case(dev, "group64_queue_overflow")
    assert r["items"] > 1.2 * r["capacity"] and r["capacity"] > BC.GROUP16_MAX, r
    assert not r["overflow"]


def test_reach_unknown_queued(dev):
    """Thin tilted splats whose det Q cancels: make_tile_reach gives up, the walk takes the whole bbox and every
    candidate tile goes through the LDS late ring.  200 000 hidden splats make the queue long enough for all of them."""
    r, V, I, _ = _run_case(dev, "unknown_queued")
    assert V == 20_000 and r["n_unknown_queued"] > 5000, r
    assert 1.2 * BC.GROUP4_MAX < r["items"] < 0.8 * BC.GROUP16_MAX and r["items"] <= r["capacity"], r


def test_reach_unknown_inline_retest(dev):
    """The same thin splats with a queue of 20 000 slots for ~200 000 items: kInlineRetest, the serial walk of both
    passes, on rectangles of unknown reach."""
    r, V, I, _ = _run_case(dev, "unknown_inline_retest")
    assert V == 20_000 == r["capacity"] and r["n_unknown_queued"] > 5000, r
    assert r["items"] > 5 * r["capacity"], r


@pytest.mark.parametrize("tiles", list(BC.TILE_BIT_FRAMES))
def test_tile_count_bits(dev, tiles):
    """Frames of 1, 15, 16, 255, 256, 4 095 and 4 096 tiles: 1, 4, 5, 8, 9, 12 and 13 sorted bits, i.e. one or two sort
    passes on either side of each digit boundary."""
    r, V, I, _ = _run_case(dev, f"tiles_{tiles}")
    assert r["num_tiles"] == tiles and V == 60_000 and I > V // 2 and not r["overflow"]


@pytest.mark.parametrize("cap", BC.WIDE_CAPS)
@pytest.mark.parametrize("tiles", list(BC.WIDE_FRAMES))
def test_more_than_16_tile_bits(dev, tiles, cap):
    """65 535 tiles (the last 16-bit count), 65 536, 65 792 and a 4097 x 16 strip: the three-pass tile sort, tile ids
    that do not fit the 16-bit key packing, the three-way width split and the edges out of a third pass, in the fused
    sort shape (6 M) and the 3-launch one (9 M)."""
    r, V, I, _ = _run_case(dev, f"wide_{tiles}_cap{cap // 1_000_000}m")
    assert r["num_tiles"] == tiles and V == 60_000 and I > V and not r["overflow"]
    assert (tiles.bit_length() > 16) == (tiles > 65535)
    assert (cap > 512 * 16384) == (cap == 9_000_000)


def test_gradients_above_65535_tiles(dev):
    """The 65 792-tile frame through the backward in default mode: the compositing backward and its zero-fill see tile
    ids above 65 535 as well."""
    name = "wide_65792_cap6m"
    c = BC.CASES[name]
    _, cloud = _cloud(name)
    gpu, orc = RT._run_pair(dev, cloud, c["w"], c["h"], 0, max_intersects=c["cap"], deterministic=False)
    V, I = RT._assert_forward_parity(gpu, orc, c["w"], c["h"], rounding_flips=True)
    assert V == 60_000 and I > V and int(gpu["u"]["tile_bounds"][0]) * int(gpu["u"]["tile_bounds"][1]) == 65792
    BK.assert_binning_properties(BK.aux_arrays(gpu["aux"], gpu["u"]["num_visible"]))
    RT._assert_grad_parity(gpu, orc, name)
