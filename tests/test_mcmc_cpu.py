"""The MCMC strategy without a GPU: the Philox known answers and the identities of the float64 restatement
(tests/mcmc_ref64.py), the sampler, the configuration, the command line and the library's symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mcmc_ref64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Random123's known answers for Philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert M.philox4x32_10(counter, key) == want


def test_philox_columns_equal_the_scalar_rounds():
    seed, step = 0x123456789ABCDEF, 77
    words = M.philox_words(seed, step, 300)
    for g in (0, 1, 63, 64, 255, 299):
        want = M.philox4x32_10((g, step, M.COUNTER_TAG, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert tuple(int(x) for x in words[g]) == want
    u = M.uniforms(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint64))
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[3] == 1.0 - 2.0 ** -25
    xi = M.xi64(5, 3, 4000)
    assert np.isfinite(xi).all() and abs(xi.mean()) < 5.0 / np.sqrt(xi.size) and abs(xi.var() - 1.0) < 5.0 * np.sqrt(
        2.0 / xi.size)


OPACITIES = (0.005, 0.3, 0.9, 0.999, 1.0 - 1e-7)


def test_relocation_identities():
    for o in OPACITIES:
        o1, coeff, _ = M.relocation64(o, 1)
        assert abs(o1 - o) <= 1e-15 and abs(coeff - 1.0) <= 1e-15
        for N in (1, 2, 5, 51):
            o_new, coeff, dabs = M.relocation64(o, N)
            assert abs((1.0 - (1.0 - o_new) ** N) - o) <= 1e-12, (o, N)
            assert 0.0 < o_new <= o and coeff > 0.0 and np.isfinite(dabs)
        assert M.relocation64(o, 60) == M.relocation64(o, 51) and M.relocation64(o, 0) == M.relocation64(o, 1)


def test_relocation_rows_agree_with_the_opacity_form():
    raw = np.array([np.log(o / (1.0 - o)) for o in OPACITIES], np.float32)
    ls = np.linspace(-4.0, 1.0, 15).reshape(5, 3).astype(np.float32)
    for N in (1, 2, 5, 51, 60):
        new_raw, new_ls = M.relocation_rows64(raw, ls, [N] * 5, 0.005)
        for g in range(5):
            o = float(M.sigmoid(np.float64(raw[g])))
            o_new, coeff, _ = M.relocation64(o, N)
            assert np.allclose(new_ls[g], ls[g].astype(np.float64) + np.log(coeff), rtol=0, atol=1e-9)
            c = min(max(o_new, 0.005), 1.0 - 2.0 ** -24)
            assert abs(new_raw[g] - np.log(c / (1.0 - c))) <= 1e-7 * max(1.0, abs(new_raw[g]))


def test_sample_by_weight_matches_numpy():
    import torch

    from brush_amd.mcmc import sample_by_weight

    rng = np.random.default_rng(2)
    w = rng.random(257).astype(np.float32)
    w[[0, 5, 6, 100, 255, 256]] = 0.0   # zero weights at the head, inside and at the tail
    u = np.concatenate([[0.0, 1.0 - 2.0 ** -53, 0.5], rng.random(5000)])
    got = sample_by_weight(torch.from_numpy(w), torch.from_numpy(u)).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, M.sample_by_weight_np(w, u))
    assert (w[got] > 0).all() and got[0] == 1 and got[1] == 254
    # the draw frequencies follow the weights (5 sigma of the binomial)
    p = w.astype(np.float64) / w.sum(dtype=np.float64)
    cnt = np.bincount(got[3:], minlength=257)
    assert (np.abs(cnt - 5000 * p) <= 5.0 * np.sqrt(5000 * p * (1 - p)) + 1.0).all()
    one = sample_by_weight(torch.tensor([0.25]), torch.tensor([0.0, 0.7, 1.0 - 2.0 ** -53], dtype=torch.float64))
    assert one.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        sample_by_weight(torch.zeros(0), torch.zeros(1))


def test_config_fields_and_cli_flags():
    from brush_amd import TrainConfig
    from brush_amd.mcmc import McmcRefineStats
    from brush_amd.train_loop import parser

    c = TrainConfig()
    assert (c.strategy, c.mcmc_cap_max, c.mcmc_noise_lr, c.mcmc_min_opacity, c.mcmc_opacity_reg, c.mcmc_scale_reg,
            c.mcmc_growth) == ("default", 1_000_000, 5e5, 0.005, 0.01, 0.01, 1.05)
    assert McmcRefineStats(3, 4).num_relocated == 3 and McmcRefineStats(3, 4).num_added == 4
    a = parser().parse_args(["scene"])
    assert a.strategy == "default" and a.cap_max == 1_000_000
    a = parser().parse_args(["scene", "--strategy", "mcmc", "--cap-max", "1500"])
    assert a.strategy == "mcmc" and a.cap_max == 1500
    with pytest.raises(SystemExit):
        parser().parse_args(["scene", "--strategy", "other"])


def test_unknown_strategy_raises_before_any_device_work():
    from brush_amd import SplatTrainer, TrainConfig

    class NoSplats:  # never touched: the strategy is checked first
        pass

    with pytest.raises(ValueError, match="strategy"):
        SplatTrainer(NoSplats(), TrainConfig(strategy="adc"))


def test_library_exports_the_mcmc_symbols():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    lib = _lib.lib()
    for name in ("brush_mcmc_inject_noise", "brush_mcmc_reg_grads", "brush_mcmc_relocation"):
        assert name in _lib.SYMBOL_NAMES and hasattr(lib, name)
    # a zero count is BRUSH_OK without touching the pointers; NULL or misaligned arguments are rejected on the host
    assert lib.brush_mcmc_inject_noise(None, None, None, None, 0, 1.0, 1, 0, None, None) == 0
    assert lib.brush_mcmc_reg_grads(None, None, 0, 0.01, 0.01, None, None, None) == 0
    assert lib.brush_mcmc_relocation(None, None, None, 0, 0.005, None, None, None) == 0
    assert lib.brush_mcmc_inject_noise(None, None, None, None, 4, 1.0, 1, 0, None, None) == -1
    assert lib.brush_mcmc_reg_grads(None, None, 4, 0.01, 0.01, None, None, None) == -1
    assert lib.brush_mcmc_relocation(None, None, None, 4, 0.005, None, None, None) == -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16  # a 16-byte aligned address inside the buffer
    assert lib.brush_mcmc_inject_noise(p + 2, p, p, p, 4, 1.0, 1, 0, None, None) == -1
    assert lib.brush_mcmc_inject_noise(p, p, p + 4, p, 4, 1.0, 1, 0, None, None) == -1  # rotation: 16 bytes
    assert lib.brush_mcmc_reg_grads(p, p, 4, 0.01, 0.01, p + 1, p, None) == -1
    assert lib.brush_mcmc_relocation(p, p, p + 2, 4, 0.005, p, p, None) == -1
    assert lib.brush_mcmc_relocation(p, p, p, 4, 0.0, p, p, None) == -1  # min_opacity outside (0, 1)
