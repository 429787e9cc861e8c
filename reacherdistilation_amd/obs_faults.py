"""Sensor faults on the student's observation in the closed loop (include/reacher_obs_faults.h): the
modes' names, the one place that turns (mode, keep_prob, seed) into an rd_obs_faults, and the stepwise
primitive ``mask_obs`` (rd_mask_obs), which calls the device functions the fused kernels inline -- a
stepwise loop {teacher forward, mask_obs, student forward on the masked row, BatchedReacher.step} steps
its envs with the fused calls' bits.

  "none"     the student reads ob
  "dropout"  tf.nn.dropout: a kept reading is ob / keep_prob, a lost one 0  (the training transform)
  "missing"  a dead sensor: a kept reading is ob, a lost one 0

Component k of the observation is kept iff u_k < keep_prob, u_k a function of (seed, env_base + i,
episode, step, k) alone.  Only the student reads the masked observation; the teacher, the rows and the
records keep the clean one.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as nat

OBS_MODES = {"none": 0, "dropout": 1, "missing": 2}   # RD_OBS_*
MODE_NAMES = {v: k for k, v in OBS_MODES.items()}
ObsFaults = nat.RdObsFaults
OB_DIM = 11


def native(mode: str, keep_prob: float, seed: int) -> nat.RdObsFaults:
    """The checked rd_obs_faults of (mode, keep_prob, seed): ValueError for an unknown mode or a keep_prob
    that is NaN or outside (0, 1]."""
    if mode not in OBS_MODES:
        raise ValueError(f"faults mode must be one of {sorted(OBS_MODES)}, got {mode!r}")
    keep_prob = float(keep_prob)
    if not 0.0 < keep_prob <= 1.0:
        raise ValueError(f"faults keep_prob must be in (0, 1], got {keep_prob}")
    return nat.RdObsFaults(mode=OBS_MODES[mode], keep_prob=keep_prob, seed=int(seed) % 2 ** 64)


def parse(faults, default_seed: int):
    """``faults`` of evaluate(faults=...) as a checked rd_obs_faults, or None for the clean query: None or
    "none"; a mode name (keep_prob 1); (mode, keep_prob) or (mode, keep_prob, seed); or a dict with those
    keys.  The seed defaults to ``default_seed``."""
    if faults is None:
        return None
    if isinstance(faults, str):
        faults = (faults,)
    if isinstance(faults, dict):
        unknown = set(faults) - {"mode", "keep_prob", "seed"}
        if unknown:
            raise ValueError(f"faults has unknown keys {sorted(unknown)}")
        faults = (faults.get("mode", "none"), faults.get("keep_prob", 1.0), faults.get("seed"))
    faults = tuple(faults)
    if not 1 <= len(faults) <= 3:
        raise ValueError("faults must be None, a mode, (mode, keep_prob[, seed]) or a dict of them")
    mode = faults[0]
    keep_prob = faults[1] if len(faults) > 1 else 1.0
    seed = faults[2] if len(faults) > 2 and faults[2] is not None else default_seed
    of = native(mode, keep_prob, seed)
    return None if of.mode == OBS_MODES["none"] else of


def mask_obs(ob: torch.Tensor, *, mode: str, keep_prob: float = 1.0, seed: int = 0, env_base: int = 0,
             episode: int = 0, step: int = 0, return_kept: bool = False):
    """seen [n, 11]: what the student reads of ob [n, 11], the observations of envs env_base ..
    env_base + n - 1 at (episode, step) (rd_mask_obs); with ``return_kept`` also kept [n, 11] uint8.
    Asynchronous on the current stream of ob's device."""
    of = native(mode, keep_prob, seed)
    if ob.device.type != "cuda":
        raise ValueError("mask_obs runs on a GPU (HIP) device only; there is no CPU path")
    o = ob.to(torch.float32).reshape(-1, OB_DIM).contiguous()
    seen = torch.empty_like(o)
    kept = torch.empty(o.shape, dtype=torch.uint8, device=o.device) if return_kept else None
    with torch.cuda.device(o.device):
        nat.check(nat.load().rd_mask_obs(ctypes.byref(of), int(env_base), o.shape[0], int(episode), int(step),
                                         nat.ptr(o), nat.ptr(seen), nat.ptr(kept) if return_kept else None,
                                         o.device.index or 0, nat.stream_handle(o.device)),
                  "rd_mask_obs")
    return (seen, kept) if return_kept else seen
