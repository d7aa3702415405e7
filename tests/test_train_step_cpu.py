"""SplatTrainer.step's decisions that need no GPU: which optimizer path a step takes, what it refuses before it touches
anything, and the one place the splats' parameters are replaced."""
import itertools

import pytest
import torch

from brush_amd import Splats
from brush_amd.train import SplatTrainer, TrainConfig, optimizer_path


def _bare_trainer(mcmc=False, depth=False, filt=False):
    t = SplatTrainer.__new__(SplatTrainer)  # no GPU state: the checks look at the configuration and the filter only
    t.config = TrainConfig(strategy="mcmc" if mcmc else "default", depth_weight=0.1 if depth else 0.0)
    t.filter3d = torch.zeros(4) if filt else None
    return t


def test_optimizer_path_of_every_combination_the_refusals_let_through():
    sync = lambda block, aux: None
    seen = {}
    for exchange, grad_sync, fused_backward, mcmc, depth, filt in itertools.product((False, True), repeat=6):
        t = _bare_trainer(mcmc, depth, filt)
        try:
            t._check_step(sync if grad_sync else None, object() if exchange else None, None, None, None,
                          object() if depth else None)
        except ValueError:
            assert exchange or grad_sync  # a single-view step refuses none of these
            continue
        if exchange:
            want = "records"
        elif grad_sync or mcmc or depth or filt:
            want = "separate"
        else:
            want = "fused" if fused_backward else "separate"
        assert optimizer_path(exchange, grad_sync, fused_backward, mcmc, depth, filt) == want
        seen[(exchange, grad_sync, fused_backward, mcmc, depth, filt)] = want
    # all 16 single-view combinations, and exchange or grad_sync alone with fused_backward either way
    assert len(seen) == 16 + 2 + 2
    assert sorted(k[2:] for k in seen if k[0] or k[1]) == [(False, False, False, False), (False, False, False, False),
                                                           (True, False, False, False), (True, False, False, False)]
    assert set(seen.values()) == {"records", "fused", "separate"}


def test_exchange_with_grad_sync_is_refused_before_anything_is_touched():
    t = _bare_trainer()
    with pytest.raises(ValueError, match="exchange and grad_sync"):
        t.step(None, None, None, 1.0, 2, lambda block, aux: None, object())
    # what is single-view still names itself first
    with pytest.raises(ValueError, match="mcmc strategy is single-view"):
        _bare_trainer(mcmc=True).step(None, None, None, exchange=object(), grad_sync=lambda block, aux: None)
    with pytest.raises(ValueError, match="poses needs view_index"):
        t.step(None, None, None, poses=object())


def test_splats_replace_parameters():
    z = torch.zeros
    given = (z((4, 3)), z((4, 4, 3)), z((4, 4)), z((4,)), z((4, 3)))
    s = Splats(*given)  # the constructor goes through the same method, on copies of what it is given
    for x, p in zip(given, (s.means, s.sh_coeffs, s.rotation, s.raw_opacity, s.log_scales)):
        assert isinstance(p, torch.nn.Parameter) and p.data_ptr() != x.data_ptr() and p.shape == x.shape
    assert tuple(s.xys_dummy.shape) == (4, 2) and s.xys_dummy.requires_grad and s.lazy_sh_owner is None
    for n in (7, 2, 0):  # grows, shrinks, empties
        old = (s.means, s.sh_coeffs, s.rotation, s.raw_opacity, s.log_scales)
        g = torch.Generator().manual_seed(n)
        # rows taken out of wider tensors and a transpose: none of them contiguous for n > 1
        new = (torch.randn((n, 5), generator=g)[:, 1:4], torch.randn((n, 4, 6), generator=g)[:, :, ::2],
               torch.randn((4, n), generator=g).t(), torch.randn((n, 2), generator=g)[:, 0],
               torch.randn((n, 6), generator=g)[:, ::2])
        assert n < 2 or not any(x.is_contiguous() for x in new)
        s.replace_parameters(*new)
        got = (s.means, s.sh_coeffs, s.rotation, s.raw_opacity, s.log_scales)
        assert s.num_splats() == n
        for o, x, p in zip(old, new, got):
            assert isinstance(p, torch.nn.Parameter) and p is not o and p.requires_grad
            assert p.is_contiguous() and p.dtype == torch.float32 and p.shape == x.shape and torch.equal(p.detach(), x)
        assert len({id(p) for p in got}) == 5 and [k for k, _ in s.named_parameters()] == [
            "means", "sh_coeffs", "rotation", "raw_opacity", "log_scales"]
        assert tuple(s.xys_dummy.shape) == (n, 2) and s.xys_dummy.requires_grad
        assert s.xys_dummy.dtype == torch.float32 and not s.xys_dummy.any()
