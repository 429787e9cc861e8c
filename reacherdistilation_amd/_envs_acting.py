"""How a student trainer's persistent envs act: what StudentMlpTrainer and StudentLstmTrainer have in
common of DAgger's teacher share, the action noise and the sensor faults (csrc/rd_acting.h keeps the
settings behind rd?_envs_set_*).

``EnvsActing`` is a mixin.  The trainer sets ``_ABI`` ("rdm" / "rdl"), calls ``_init_acting()`` once it has
its handle (``_lib``, ``_h``, ``device``) and ``_attach_acting()`` from attach_envs; its own set_* overrides
add only the sentence on what the setting leaves unchanged for that student.  A seed left to default follows
the envs' seed, whatever attach_envs sets it to.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as nat
from . import action_noise as an
from . import obs_faults as obf


class EnvsActing:
    _ABI = ""

    def _init_acting(self):
        self._envs_seed, self._coin_seed = 0, None   # set_teacher_share
        self._noise, self._noise_seed, self._actions = ("none", 1.0), None, None   # set_action_noise, actions
        self._faults, self._faults_seed = ("none", 1.0), None   # set_obs_faults

    def _acting_call(self, name: str, *args):
        name = f"{self._ABI}_envs_{name}"
        nat.check(getattr(self._lib, name)(self._h, *args), name)

    def _attach_acting(self, seed: int, steps: int, n_envs: int, actions: bool):
        """attach_envs' part: the settings whose seed follows the envs' again, and the actions buffer"""
        self._envs_seed = int(seed)
        if self._coin_seed is None:
            self._set_share(self.teacher_share)
        if self._noise_seed is None:
            self._set_noise()
        if self._faults_seed is None:
            self._set_faults()
        if actions or self._actions is not None:
            self._actions = torch.zeros(steps, n_envs, 2, dtype=torch.float32, device=self.device)
            self._acting_call("bind_actions", nat.ptr(self._actions), steps * n_envs)

    # -- action noise in the envs calls ---------------------------------------------------------
    def set_action_noise(self, mode: str = "none", scale: float = 1.0, seed: int | None = None):
        """Sample the acting policy in act_envs / rollout_envs / step_envs from the next call on
        (rd?_envs_set_action_noise; action_noise.py has the modes), under "student" (with the teacher
        share's coin as it is) and under "teacher" (DART's noisy expert): the action handed to env.step
        is mean + scale (exp(logstd) | 1) xi of whoever acts at that step, xi a function of (seed,
        env_base + i, episode, step) alone.  Only that action changes.  ``seed``: the noise's key
        (default: the envs' seed, whatever attach_envs sets it to).  "none" (the default) is the plain
        call.  evaluate() never reads this setting.  A captured call keeps the noise it was captured
        with."""
        an.native(mode, scale, 0)   # ValueError before anything is kept
        self._noise, self._noise_seed = (mode, float(scale)), None if seed is None else int(seed)
        self._set_noise()

    def _set_noise(self):
        nz = an.native(*self._noise, self._envs_seed if self._noise_seed is None else self._noise_seed)
        self._acting_call("set_action_noise", ctypes.byref(nz))

    @property
    def action_noise(self) -> dict:
        """dict(mode, scale, seed): the handle's setting (rd?_envs_action_noise)"""
        nz = nat.RdActionNoise()
        self._acting_call("action_noise", ctypes.byref(nz))
        return dict(mode=an.MODE_NAMES[nz.mode], scale=float(nz.scale), seed=int(nz.seed))

    @property
    def actions(self):
        """[accum_steps, n, 2] f32, the trainer's own and rewritten by every envs call of either actor:
        the action that stepped env i at the call's k-th step (the acting mean when the noise is off);
        rows past a shorter call's ``steps`` keep their old values.  None unless attach_envs(...,
        actions=True) asked for it."""
        return self._actions

    # -- sensor faults on what the student reads in the envs calls ---------------------------------
    def set_obs_faults(self, mode: str = "none", keep_prob: float = 1.0, seed: int | None = None):
        """Mask the observations the student reads in act_envs / rollout_envs / step_envs ("student") from
        the next call on (rd?_envs_set_obs_faults; obs_faults.py has the modes): a component is kept iff
        u < keep_prob, u a function of (seed, env_base + i, episode, step, component) alone; "dropout"
        scales a kept reading by 1 / keep_prob as the training dropout does, "missing" leaves it.  Only
        the student's pdflat, and through it the trajectory, changes: the teacher reads the clean
        observation, and "teacher" calls ignore the setting.  ``seed``: the mask's key (default: the
        envs' seed, whatever attach_envs sets it to).  "none" (the default) is the plain call.
        evaluate() never reads this setting.  A captured call keeps the faults it was captured with."""
        obf.native(mode, keep_prob, 0)   # ValueError before anything is kept
        self._faults, self._faults_seed = (mode, float(keep_prob)), None if seed is None else int(seed)
        self._set_faults()

    def _set_faults(self):
        of = obf.native(*self._faults, self._envs_seed if self._faults_seed is None else self._faults_seed)
        self._acting_call("set_obs_faults", ctypes.byref(of))

    def obs_faults(self) -> dict:
        """dict(mode, keep_prob, seed): the handle's setting (rd?_envs_obs_faults)"""
        of = nat.RdObsFaults()
        self._acting_call("obs_faults", ctypes.byref(of))
        return dict(mode=obf.MODE_NAMES[of.mode], keep_prob=float(of.keep_prob), seed=int(of.seed))

    # -- DAgger's beta-mixture in the student-stepped envs calls ----------------------------------
    def set_teacher_share(self, beta: float, seed: int | None = None):
        """The teacher's share beta in [0, 1] of the env steps in act_envs / rollout_envs / step_envs
        ("student") from the next call on (rd?_envs_set_teacher_share; "teacher" calls ignore it): per env
        and step a coin, a function of (seed, env_base + i, episode, step) alone -- Philox, word 3 of the
        counter = 0x80000000 | step, u < beta -- hands the teacher's mean to env.step instead of the
        student's; everything else of the step, and the training, is the student call's.  ``seed``:
        the coins' key (default: the envs' seed, whatever attach_envs sets it to).  beta = 0 (the
        default) is the plain student call.  A captured call keeps the beta it was captured with."""
        beta = float(beta)
        if not 0.0 <= beta <= 1.0:
            raise ValueError(f"beta must be in [0, 1], got {beta}")
        self._coin_seed = None if seed is None else int(seed)
        self._set_share(beta)

    def _set_share(self, beta: float):
        seed = self._envs_seed if self._coin_seed is None else self._coin_seed
        self._acting_call("set_teacher_share", beta, seed % 2 ** 64)

    @property
    def teacher_share(self) -> float:
        return float(getattr(self._lib, f"{self._ABI}_envs_teacher_share")(self._h))
