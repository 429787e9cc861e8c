"""Action noise of the acting policy in the students' closed loop (include/reacher_action_noise.h):
the modes' names, the one place that turns (mode, scale, seed) into an rd_action_noise, and the
stepwise primitive ``perturb_actions`` (rd_perturb_actions), which calls the device function the fused
kernels inline -- a stepwise loop {forward, perturb_actions, BatchedReacher.step} steps its envs with
the fused calls' bits.

  "none"    the mean acts
  "policy"  a = mean + scale exp(logstd) xi   (the policy's own Gaussian: baselines' stochastic=True)
  "fixed"   a = mean + scale xi               (DART's isotropic sigma = scale)

xi is a pair of normal draws, a function of (seed, env_base + i, episode, step) alone.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _native as nat

NOISE_MODES = {"none": 0, "policy": 1, "fixed": 2}   # RD_NOISE_*
MODE_NAMES = {v: k for k, v in NOISE_MODES.items()}


def native(mode: str, scale: float, seed: int) -> nat.RdActionNoise:
    """The checked rd_action_noise of (mode, scale, seed): ValueError for an unknown mode or a scale that
    is NaN, negative or infinite."""
    if mode not in NOISE_MODES:
        raise ValueError(f"noise mode must be one of {sorted(NOISE_MODES)}, got {mode!r}")
    scale = float(scale)
    if not (scale >= 0.0 and math.isfinite(scale)):
        raise ValueError(f"noise scale must be a finite value >= 0, got {scale}")
    return nat.RdActionNoise(mode=NOISE_MODES[mode], scale=scale, seed=int(seed) % 2 ** 64)


def perturb_actions(pdflat: torch.Tensor, *, mode: str, scale: float = 1.0, seed: int = 0, env_base: int = 0,
                    episode: int = 0, step: int = 0, return_xi: bool = False):
    """actions [n, 2] of envs env_base .. env_base + n - 1 at (episode, step) from their acting pdflat
    [n, 4] = mean | logstd (rd_perturb_actions); with ``return_xi`` also the draws xi [n, 2].
    Asynchronous on the current stream of pdflat's device."""
    nz = native(mode, scale, seed)
    if pdflat.device.type != "cuda":
        raise ValueError("perturb_actions runs on a GPU (HIP) device only; there is no CPU path")
    p = pdflat.to(torch.float32).reshape(-1, 4).contiguous()
    act = torch.empty(p.shape[0], 2, dtype=torch.float32, device=p.device)
    xi = torch.empty_like(act) if return_xi else None
    with torch.cuda.device(p.device):
        nat.check(nat.load().rd_perturb_actions(ctypes.byref(nz), int(env_base), p.shape[0], int(episode), int(step),
                                                nat.ptr(p), nat.ptr(act), nat.ptr(xi) if return_xi else None,
                                                p.device.index or 0, nat.stream_handle(p.device)),
                  "rd_perturb_actions")
    return (act, xi) if return_xi else act
