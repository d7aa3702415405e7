"""CPU-side checks of pruning by rendered contribution: the hand-made cases are threshold-free, the float64 reference
checks itself (exact cases, wrong references, a float32 restatement inside the allowance), the pure-torch layer
(prune_mask, Splats.select, Contributions.accumulate), the trainer's configuration and both command lines, and the
library: argument validation of brush_render_contributions and the resources of k_contribution_quad."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from tests import contrib_cases as CC
from tests import contrib_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in CC.all_cases()}


@pytest.fixture(scope="module")
def refs(cases):
    """One reference walk per case, shared and left unchanged."""
    return {name: R.walk(c, want_decisions=True) for name, c in cases.items()}


# ---------------------------------------------------------------------------- the cases and the reference
def test_case_list_covers_the_shapes(cases):
    assert cases["empty"]["num_isect"] == 0
    assert [cases[f"batch_{k}"]["num_isect"] for k in (64, 65, 129)] == [64, 65, 129]
    assert (cases["ragged_17x9"]["w"], cases["ragged_17x9"]["h"]) == (17, 9)
    assert cases["four_tiles"]["tile_bins"].shape == (2, 2, 2)
    assert 180 <= cases["random_200"]["num_visible"] <= 220 and cases["random_200"]["tile_bins"].shape == (2, 3, 2)
    for name in ("batch_64", "saturating", "random_200", "four_tiles"):  # id maps that are not the identity, with gaps
        c = cases[name]
        g = c["g_from_c"][:c["num_visible"]]
        assert c["n"] > c["num_visible"] and not np.array_equal(g, np.arange(c["num_visible"]))
    for name, c in cases.items():
        if name != "clamped":
            assert c["num_visible"] == 0 or float(c["projected"][:c["num_visible"], 8].max()) <= 0.9, name


def test_every_case_is_threshold_free(cases, refs):
    """No alpha test, sigma test or stop test of any case lies within 8 allowances of its threshold: the device must
    reproduce the reference's hit and stop counts exactly, and the GPU test leaves no entry out."""
    for name, ref in refs.items():
        d = ref["decisions"]
        worst = float(d.min()) if d.size else np.inf
        print(f"{name}: {d.size} decisions, nearest {worst:.3g} allowances")
        assert worst > 8.0, (name, worst)


def test_reference_shapes_of_the_directed_cases(cases, refs):
    r = refs["saturating"]
    c = cases["saturating"]
    g = c["g_from_c"]
    assert int(r["stops"].sum()) == 256 and int(r["stops"][g[5]]) == 256  # one stopper per pixel: the sixth record
    assert int(r["hits"][g[5]]) == 0 and all(int(r["hits"][g[k]]) == 256 for k in range(5))
    assert not r["touched"][g[6:106]].any()  # the hundred records behind are never walked
    assert np.all(r["last"] == 4)
    r = refs["clamped"]
    assert float(r["max"][0]) == R.CLAMP and int(r["stops"][1]) == 1 and float(r["max"][2]) == R.CLAMP
    r = refs["quadrant_skip"]
    assert 20 < int(r["hits"][0]) < 40  # reach ~3.1 px around (3.5, 3.5): quadrant 0 only
    r = refs["empty"]
    assert not r["touched"].any() and not r["alpha"].any()
    # rows of ids outside the lists stay zero
    for name, ref in refs.items():
        c = cases[name]
        used = np.zeros(c["n"], bool)
        used[c["g_from_c"][:c["num_visible"]]] = True
        for k in ("max", "sum", "hits", "stops"):
            assert not ref[k][~used].any(), (name, k)


def test_exact_cases(cases, refs):
    """The float32 restatement of the kernel's arithmetic gives the exact bits the issue names."""
    emu = R.emulate32(cases["exact_single"])
    assert np.float32(emu["max"][0]).view(np.uint32) == np.float32(CC.EXACT_O).view(np.uint32)
    assert int(emu["hits"][0]) == int(refs["exact_single"]["hits"][0]) > 0
    emu = R.emulate32(cases["exact_pair"])
    want = np.float32(0.25) * (np.float32(1.0) - np.float32(0.25))
    assert np.float32(emu["max"][1]).view(np.uint32) == np.float32(want).view(np.uint32)
    assert np.float32(emu["max"][0]).view(np.uint32) == np.float32(0.25).view(np.uint32)
    assert float(refs["exact_pair"]["max"][1]) == float(want)


def test_float32_restatement_is_inside_the_allowance(cases, refs):
    for name, c in cases.items():
        g = R.gate(R.emulate32(c), refs[name])
        assert R.passes(g), (name, g)


def test_each_wrong_reference_is_rejected_somewhere(cases):
    """Each mutation changes the result beyond tolerance on at least one case (and where it does, the gate says so)."""
    emus = {name: R.emulate32(c) for name, c in cases.items()}
    for m in R.MUTATIONS:
        rejected = [name for name, c in cases.items() if not R.passes(R.gate(emus[name], R.walk(c, mutate=m)))]
        print(m, "rejected on", rejected)
        assert rejected, m
    assert not R.passes(R.gate(emus["clamped"], R.walk(cases["clamped"], mutate="noclamp")))
    assert not R.passes(R.gate(emus["saturating"], R.walk(cases["saturating"], mutate="stop_as_hit")))


# ---------------------------------------------------------------------------- the pure-torch layer
def _contrib(mx, sm, hits, stops, views=1):
    import torch

    from brush_amd.contribution import Contributions

    return Contributions(torch.tensor(mx, dtype=torch.float32), torch.tensor(sm, dtype=torch.float64),
                         torch.tensor(hits, dtype=torch.int64), torch.tensor(stops, dtype=torch.int64), views)


def test_prune_mask_rules():
    from brush_amd import prune_mask

    c = _contrib([0.5, 0.0, 0.0, 0.2, 0.009], [1.0, 0.0, 0.0, 3.0, 0.5], [3, 0, 0, 1, 9], [0, 0, 2, 0, 0])
    assert prune_mask(c, min_max=0.0).tolist() == [False, True, False, False, False]  # stops alone keep a splat
    assert prune_mask(c, min_max=0.01).tolist() == [False, True, True, False, True]
    assert prune_mask(c, min_max=0.2).tolist() == [False, True, True, False, True]    # strict: max < t
    assert prune_mask(c, keep_fraction=0.4).tolist() == [False, True, True, False, True]  # ceil(2.0) = 2 largest by max
    assert prune_mask(c, keep_fraction=0.41).tolist() == [False, True, True, False, False]  # ceil(2.05) = 3
    assert prune_mask(c, keep_fraction=0.4, by="sum").tolist() == [False, True, True, False, True]
    assert prune_mask(c, keep_fraction=0.0).all() and not prune_mask(c, keep_fraction=1.0).any()
    # ties are broken by lower index: the zeros of rows 1 and 2 tie, row 1 is kept first
    assert prune_mask(c, keep_fraction=0.8).tolist() == [False, False, True, False, False]
    tie = _contrib([0.3, 0.3, 0.3, 0.3], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0])
    assert prune_mask(tie, keep_fraction=0.5).tolist() == [False, False, True, True]


def test_prune_mask_bad_arguments():
    from brush_amd import prune_mask

    c = _contrib([0.5], [1.0], [1], [0])
    with pytest.raises(ValueError, match="exactly one"):
        prune_mask(c)
    with pytest.raises(ValueError, match="exactly one"):
        prune_mask(c, min_max=0.1, keep_fraction=0.5)
    with pytest.raises(ValueError, match="min_max"):
        prune_mask(c, min_max=-0.1)
    with pytest.raises(ValueError, match="min_max"):
        prune_mask(c, min_max=float("nan"))
    with pytest.raises(ValueError, match="keep_fraction"):
        prune_mask(c, keep_fraction=1.5)
    with pytest.raises(ValueError, match="by must be"):
        prune_mask(c, keep_fraction=0.5, by="mean")


def test_contributions_accumulate():
    a = _contrib([0.5, 0.1], [1.0, 0.25], [3, 1], [0, 2], views=2)
    b = _contrib([0.2, 0.4], [0.5, 0.5], [1, 0], [1, 0], views=1)
    c = a.accumulate(b)
    assert c.max.tolist() == [0.5, pytest.approx(0.4)] and c.sum.tolist() == [1.5, 0.75]
    assert c.hits.tolist() == [4, 1] and c.stops.tolist() == [1, 2] and c.views == 3
    assert a.max.tolist() == [0.5, pytest.approx(0.1)]  # a new object: the operands keep their values
    with pytest.raises(ValueError, match="cannot accumulate"):
        a.accumulate(_contrib([0.1], [0.1], [1], [0]))


def test_splats_select_on_cpu():
    import torch

    from brush_amd import Splats

    g = torch.Generator().manual_seed(1)
    s = Splats(torch.randn(5, 3, generator=g), torch.randn(5, 4, 3, generator=g), torch.randn(5, 4, generator=g),
               torch.randn(5, generator=g), torch.randn(5, 3, generator=g))
    a = s.select(torch.tensor([True, False, True, True, False]))
    assert a.num_splats() == 3 and a.means.device.type == "cpu" and a.xys_dummy.shape == (3, 2)
    for k in ("means", "sh_coeffs", "rotation", "raw_opacity", "log_scales"):
        assert torch.equal(getattr(a, k), getattr(s, k)[[0, 2, 3]]), k
    b = s.select(torch.tensor([4, 1]))
    assert torch.equal(b.means, s.means[[4, 1]]) and isinstance(b.means, torch.nn.Parameter)
    assert s.select(torch.zeros(5, dtype=torch.bool)).num_splats() == 0
    assert s.num_splats() == 5  # the source is untouched
    with pytest.raises(ValueError, match="boolean"):
        s.select(torch.tensor([True, False]))
    with pytest.raises(ValueError, match="outside"):
        s.select(torch.tensor([5]))
    with pytest.raises(ValueError, match="must be a boolean"):
        s.select(torch.tensor([0.5]))


# ---------------------------------------------------------------------------- configuration and command lines
def test_train_config_validation_messages():
    from brush_amd import TrainConfig

    assert TrainConfig().check_contribution_prune() == ()
    assert TrainConfig(contribution_prune_at=(0, 40, 41)).check_contribution_prune() == (0, 40, 41)
    assert TrainConfig().contribution_prune_min == 0.01
    with pytest.raises(ValueError, match="steps must be >= 0, got -1"):
        TrainConfig(contribution_prune_at=(-1,)).check_contribution_prune()
    with pytest.raises(ValueError, match="strictly increasing, got 40 after 40"):
        TrainConfig(contribution_prune_at=(40, 40)).check_contribution_prune()
    with pytest.raises(ValueError, match="integer steps, got 1.5"):
        TrainConfig(contribution_prune_at=(1.5,)).check_contribution_prune()
    with pytest.raises(ValueError, match="integer steps, got True"):
        TrainConfig(contribution_prune_at=(True,)).check_contribution_prune()
    with pytest.raises(ValueError, match="a tuple of steps"):
        TrainConfig(contribution_prune_at=40).check_contribution_prune()
    with pytest.raises(ValueError, match=r"contribution_prune_min must be in \[0, 1\], got 1.5"):
        TrainConfig(contribution_prune_at=(4,), contribution_prune_min=1.5).check_contribution_prune()


def test_mcmc_and_exchange_refusals():
    from brush_amd import TrainConfig
    from brush_amd.train_loop import TrainLoop

    class Exchange:
        def __init__(self, world):
            self.world = world

    cfg = TrainConfig(contribution_prune_at=(10,))
    cfg.check()
    cfg.check(multi_rank=False)
    assert cfg.check_contribution_prune() == (10,)
    TrainConfig(strategy="mcmc").check(multi_rank=True)  # nothing asked, nothing refused
    assert TrainConfig(strategy="mcmc").check_contribution_prune() == ()
    with pytest.raises(ValueError, match="multi-rank exchange"):
        cfg.check(multi_rank=True)
    with pytest.raises(ValueError, match="strategy='mcmc'"):
        TrainConfig(strategy="mcmc", contribution_prune_at=(10,)).check()
    # TrainLoop takes multi_rank from its exchange's world size: one rank is let through, as far as the dataset (None)
    with pytest.raises(AttributeError, match="train"):
        TrainLoop(None, cfg, steps=20, exchange=Exchange(1), device="cpu")
    with pytest.raises(ValueError, match="multi-rank exchange"):
        TrainLoop(None, cfg, steps=20, exchange=Exchange(2))
    # at construction, before anything touches the dataset or a device
    with pytest.raises(ValueError, match="strategy='mcmc'"):
        TrainLoop(None, TrainConfig(strategy="mcmc", contribution_prune_at=(10,)), steps=20)
    with pytest.raises(ValueError, match="multi-rank exchange"):
        TrainLoop(None, cfg, steps=20, exchange=Exchange(8))
    with pytest.raises(ValueError, match="strictly increasing"):
        TrainLoop(None, TrainConfig(contribution_prune_at=(5, 3)), steps=20)


def test_both_parsers(capsys):
    from brush_amd import prune, train_loop

    a = train_loop.parser().parse_args(["scene", "--contribution-prune-at", "16000,24000", "--contribution-prune-min",
                                        "0.02"])
    assert train_loop.parse_prune_steps(a.contribution_prune_at) == (16000, 24000) and a.contribution_prune_min == 0.02
    d = train_loop.parser().parse_args(["scene"])
    assert d.contribution_prune_at is None and d.contribution_prune_min == 0.01
    with pytest.raises(ValueError, match="steps separated by commas"):
        train_loop.parse_prune_steps("100,x")
    for argv in (["scene", "--contribution-prune-at", "5,5"],
                 ["scene", "--contribution-prune-at", "5", "--strategy", "mcmc"]):
        with pytest.raises(SystemExit):
            train_loop.main(argv)
    capsys.readouterr()

    p = prune.parser().parse_args(["in.ply", "scene"])
    assert prune.rule_from_args(p) == {"min_max": 0.01} and p.views == "train" and not p.antialiased
    p = prune.parser().parse_args(["in.ply", "scene", "--keep-fraction", "0.25", "--by", "sum", "--views", "all",
                                   "--export", "o.ply", "--json", "o.json", "--eval-split-every", "8",
                                   "--max-resolution", "800", "--no-undistort", "--format", "colmap", "--antialiased"])
    assert prune.rule_from_args(p) == {"keep_fraction": 0.25, "by": "sum"}
    assert (p.views, p.export, p.json, p.eval_split_every, p.max_resolution, p.no_undistort, p.format) == \
        ("all", "o.ply", "o.json", 8, 800, True, "colmap")
    assert prune.rule_from_args(prune.parser().parse_args(["a", "b", "--min-contribution", "0"])) == {"min_max": 0.0}
    with pytest.raises(ValueError, match="two rules"):
        prune.rule_from_args(prune.parser().parse_args(["a", "b", "--min-contribution", "0.1", "--keep-fraction", "0.5"]))
    with pytest.raises(ValueError, match="keep-fraction"):
        prune.rule_from_args(prune.parser().parse_args(["a", "b", "--keep-fraction", "2"]))


# ---------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_entry_point_validates_before_any_device_work(lib):
    from brush_amd import _lib

    u = _lib.BrushUniforms()
    u.img_size[:] = [17, 9]
    u.tile_bounds[:] = [2, 1]
    aux = _lib.BrushAux()
    fake = 0x1000  # never dereferenced on the host: every call below is refused before a launch
    for name in ("projected_splats", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid", "num_visible",
                 "final_index"):
        setattr(aux, name, fake)
    aux.max_intersects = 8
    call = lib.brush_render_contributions
    ok_args = [C.byref(u), C.byref(aux), None, fake, fake, None, 4, None]
    for i in (0, 1, 3, 4):  # uniforms, aux, max_bits, counts
        args = list(ok_args)
        args[i] = None
        assert call(*args) == -1, i
    assert call(C.byref(u), C.byref(aux), fake, fake, fake, None, 4, None) == -1   # out_img without mismatch
    assert call(C.byref(u), C.byref(aux), None, fake, fake, fake, 4, None) == -1   # mismatch without out_img
    assert call(C.byref(u), C.byref(aux), None, fake, fake + 4, None, 4, None) == -1  # counts: 8-byte aligned
    assert call(C.byref(u), C.byref(aux), fake + 4, fake, fake, fake, 4, None) == -1  # out_img: 16-byte aligned
    for name in ("projected_splats", "tile_bins", "compact_gid_from_isect", "global_from_compact_gid", "num_visible"):
        setattr(aux, name, None)
        assert call(*ok_args) == -1, name
        setattr(aux, name, fake)
    aux.final_index = None  # needed by the self-check only
    assert call(C.byref(u), C.byref(aux), fake, fake, fake, fake, 4, None) == -1
    assert call(C.byref(u), C.byref(aux), None, fake, fake, None, 0, None) == 0  # n = 0: nothing to do, no launch
    aux.max_intersects = 0
    assert call(*ok_args) == -1
    aux.max_intersects = 8
    u.tile_bounds[:] = [1, 1]  # not the bounds of 17 x 9
    assert call(*ok_args) == -1
    u.tile_bounds[:] = [2, 1]
    u.img_size[:] = [0, 9]
    assert call(*ok_args) == -1


def test_contribution_kernel_static_lds_and_no_spills(lib):
    """One kernel, no spills, no scratch, and the static LDS the .hip pins with a static_assert: 4 waves x 64 records x
    32 bytes."""
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_contribution_quad")
    assert len(res) == 1, sorted(res)
    (name, r), = res.items()
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name
    assert r["group_segment_fixed_size"] == 8192, name
    walk = open(os.path.join(ROOT, "brush_amd", "csrc", "replay_walk.hpp")).read()  # the staged record is the shared walk's
    assert "static_assert(sizeof(ReplayRec) * kTilesPerBlock * kBatch == 8192" in walk
    # a kernel of its own: the forward's instantiations stay three (tests/test_host_cpu.py counts them)
    assert "k_rasterize" not in name
