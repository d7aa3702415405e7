"""MCMC densification with a fixed splat budget ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et
al. 2024; gsplat's MCMCStrategy is the model) — the alternative to SplatTrainer.refine_splats chosen with
TrainConfig.strategy = "mcmc".

Per step (SplatTrainer.step): the opacity / scale regularisers enter the gradients before Adam (brush_mcmc_reg_grads) and
every mean takes a small noise step shaped by its covariance (brush_mcmc_inject_noise).  Per refinement (`refine`,
periodic, plain torch like refine_splats): dead splats are relocated onto live ones and the count grows by
TrainConfig.mcmc_growth up to TrainConfig.mcmc_cap_max, both with the opacity / scale correction of the paper's Eq. 9
(brush_mcmc_relocation).  No gradient statistic, no optimizer reset, no opacity reset.

The two pure pieces are callable on their own: `sample_by_weight` and `relocation`.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch

from . import _lib

PARAMS = ("means", "log_scales", "rotation", "raw_opacity", "sh_coeffs")  # Splats' names, in the moment segments' order


@dataclass
class McmcRefineStats:
    num_relocated: int
    num_added: int


def sample_by_weight(weights: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Indices drawn with probability proportional to `weights` [n] (>= 0, not all 0) from uniforms `u` in [0, 1): the
    inverse of the float64 cumulative sum.  (torch.multinomial stops at 2^24 categories.)  A zero-weight entry is
    never drawn: the target u * total stays below the total, and the search takes the first entry whose cumulative
    sum exceeds it."""
    if weights.dim() != 1 or weights.numel() == 0:
        raise ValueError("weights must be a non-empty vector")
    cdf = torch.cumsum(weights.to(torch.float64), 0)
    total = cdf[-1]
    below = torch.nextafter(total, torch.zeros_like(total))
    target = torch.minimum(u.to(torch.float64) * total, below)
    idx = torch.searchsorted(cdf, target, right=True)
    return idx.clamp_(max=weights.numel() - 1)


def relocation(raw_opacity: torch.Tensor, log_scales: torch.Tensor, ratio: torch.Tensor,
               min_opacity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(new raw opacity [m], new log-scales [m,3]) of rows split into `ratio` [m] copies each (brush_mcmc_relocation)."""
    assert raw_opacity.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    m = int(raw_opacity.shape[0])
    if tuple(log_scales.shape) != (m, 3) or tuple(ratio.shape) != (m,):
        raise ValueError(f"expected [m], [m,3], [m], got {tuple(raw_opacity.shape)} / {tuple(log_scales.shape)} / "
                         f"{tuple(ratio.shape)}")
    raw_opacity, log_scales = raw_opacity.contiguous().float(), log_scales.contiguous().float()
    ratio = ratio.to(torch.int32).contiguous()
    new_raw, new_scales = torch.empty_like(raw_opacity), torch.empty_like(log_scales)
    with torch.cuda.device(raw_opacity.device):
        _lib.check(_lib.lib().brush_mcmc_relocation(raw_opacity.data_ptr(), log_scales.data_ptr(), ratio.data_ptr(), m,
                                                    float(min_opacity), new_raw.data_ptr(), new_scales.data_ptr(),
                                                    _lib.current_stream()), "brush_mcmc_relocation")
    return new_raw, new_scales


def reg_grads(raw_opacity, log_scales, n: int, opacity_reg: float, scale_reg: float, v_opac, v_scales, stream):
    _lib.check(_lib.lib().brush_mcmc_reg_grads(raw_opacity.data_ptr(), log_scales.data_ptr(), n, float(opacity_reg),
                                               float(scale_reg), v_opac.data_ptr(), v_scales.data_ptr(), stream),
               "brush_mcmc_reg_grads")


def inject_noise(means, log_scales, rotation, raw_opacity, n: int, scale: float, seed: int, step: int, stream,
                 xi_out=None):
    _lib.check(_lib.lib().brush_mcmc_inject_noise(means.data_ptr(), log_scales.data_ptr(), rotation.data_ptr(),
                                                  raw_opacity.data_ptr(), n, float(scale),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF,
                                                  None if xi_out is None else xi_out.data_ptr(), stream),
               "brush_mcmc_inject_noise")


def moment_segments(moment: torch.Tensor, n: int, ncoef: int) -> List[torch.Tensor]:
    """[n, width] views of the five segments [means|log_scales|quats|raw_opac|sh] of a moment array."""
    out, off = [], 0
    for width in (3, 3, 4, 1, 3 * ncoef):
        out.append(moment[off:off + n * width].view(n, width))
        off += n * width
    return out


def _split(params: dict, idx: torch.Tensor, min_opacity: float):
    """Writes the relocated opacity / scale of the sampled rows `idx` (each split into its draw count + 1 copies)."""
    n = params["raw_opacity"].shape[0]
    ratio = torch.bincount(idx, minlength=n)[idx] + 1
    new_raw, new_scales = relocation(params["raw_opacity"][idx], params["log_scales"][idx], ratio, min_opacity)
    params["raw_opacity"][idx] = new_raw      # duplicates of an index carry the same ratio, so the same values
    params["log_scales"][idx] = new_scales


@torch.no_grad()
def refine(trainer, splats) -> McmcRefineStats:
    """One MCMC refinement on the post-step parameters: relocate the dead splats, then grow towards the cap."""
    c = trainer.config
    dev = splats.means.device
    p = {k: getattr(splats, k).detach() for k in PARAMS}
    n, ncoef = int(p["means"].shape[0]), int(p["sh_coeffs"].shape[1])
    m1, m2 = moment_segments(trainer.moment1, n, ncoef), moment_segments(trainer.moment2, n, ncoef)

    # 1. relocate
    opac = torch.sigmoid(p["raw_opacity"])
    dead = opac <= c.mcmc_min_opacity
    dead_idx, live_idx = torch.nonzero(dead).squeeze(1), torch.nonzero(~dead).squeeze(1)
    n_dead = int(dead_idx.numel())
    num_relocated = 0
    if n_dead > 0 and live_idx.numel() > 0:
        u = torch.rand(n_dead, generator=trainer.rng, device=dev, dtype=torch.float64)
        src = live_idx[sample_by_weight(opac[live_idx], u)]
        _split(p, src, c.mcmc_min_opacity)
        for k in PARAMS:
            p[k][dead_idx] = p[k][src]
        for seg in m1 + m2:  # a dead splat's moments describe a place it has left
            seg[src] = 0.0
            seg[dead_idx] = 0.0
        num_relocated = n_dead

    # 2. grow
    n_target = min(int(c.mcmc_cap_max), int(c.mcmc_growth * n))
    num_added = max(n_target - n, 0)
    if num_added > 0:
        u = torch.rand(num_added, generator=trainer.rng, device=dev, dtype=torch.float64)
        src = sample_by_weight(torch.sigmoid(p["raw_opacity"]), u)
        _split(p, src, c.mcmc_min_opacity)
        new = {k: torch.cat([p[k], p[k][src]], 0) for k in PARAMS}
        moments = []
        for segs in (m1, m2):
            parts = []
            for seg in segs:
                seg[src] = 0.0
                parts += [seg.reshape(-1), torch.zeros(num_added * seg.shape[1], dtype=seg.dtype, device=dev)]
            moments.append(torch.cat(parts))
        trainer.moment1, trainer.moment2 = moments
        splats.replace_parameters(**new)
        trainer._reset_stats(n_target, dev)  # (the moments above are kept: no optimizer reset)
    trainer.invalidate_cached_rotation()
    return McmcRefineStats(num_relocated, num_added)
