"""Host layer of the reference's own MLP student (include/reacher_student_mlp.h).

``StudentMlpTrainer`` is the 'MLP' scope of the reference's mlp_train.py (:35-80): the
graph ``student_mlp_graph`` (student_nn.py:51-57, 16 -> 24 -> 128 -> 128 -> 32 -> 4 with a
state-dependent log-std), ``kl_loss`` (loss.py:3-13) or action-MSE, and TF1 Adam, run by the
HIP kernels in csrc/student_mlp.hip.  ``rows()`` is the input concat of mlp_train.py:50-52
(dropout(ob) | prev_pdflat | prev_rew; the dropout itself runs inside the kernel).

Multi-GPU: rows sharded contiguously (dist.shard); one all_reduce(SUM) of the flat
24,380-float gradient per optimiser step.  The persistent envs (attach_envs / act_envs /
rollout_envs / step_envs: batched on-policy distillation, rdm_step_envs) are single-GPU.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from . import action_noise as an
from . import obs_faults as obf
from ._envs_acting import EnvsActing
from .config import OBSPACE_SHAPE, PDFLAT_SHAPE
from .dist import allreduce_sum_
from .distill import EvalResult

P = nat.P
I32, I64, U64, F32, INT = nat.I32, nat.I64, nat.U64, nat.F32, nat.INT

DIMS = (16, 24, 128, 128, 32, 4)          # student_nn.py:51-57
N_PARAMS = sum(a * b + b for a, b in zip(DIMS[:-1], DIMS[1:]))   # 24,380
IN_DIM = OBSPACE_SHAPE + PDFLAT_SHAPE + 1
LOSSES = {"mse": 0, "kl": 1}
DTYPES = {"f32": 0, "bf16": 1}            # RDM_DTYPE_*


class RdmConfig(ctypes.Structure):
    _fields_ = [("loss", I32), ("lr", F32), ("beta1", F32), ("beta2", F32), ("eps", F32), ("grid", I32),
                ("metrics_len", I32), ("keep_prob", F32), ("seed", U64), ("row_base", I64)]


class RdmEvalConfig(ctypes.Structure):
    _fields_ = [("n_envs", I64), ("env_base", I64), ("seed", U64), ("episodes", I32), ("first_episode", I32),
                ("grid", I32), ("draws", P)]


class RdmEnvsConfig(ctypes.Structure):
    _fields_ = [("n_envs", I64), ("env_base", I64), ("seed", U64), ("grid", I32)]


ACT_WITH = {"teacher": 0, "student": 1}   # RDM_ACT_*
_ENVS_CALL = (INT, [P, INT, INT, P, P, P, P])

nat.register({
    "rdm_envs_attach": (INT, [P, ctypes.POINTER(RdmEnvsConfig)]),
    "rdm_envs_reset": (INT, [P]),
    "rdm_envs_act": _ENVS_CALL,
    "rdm_rollout_envs": _ENVS_CALL,
    "rdm_step_envs": _ENVS_CALL,
    "rdm_envs_get_state": (INT, [P, P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
    **nat.envs_acting("rdm"),
    "rdm_envs_bind_stepped_with": (INT, [P, P, I64]),
    "rdm_evaluate_noisy": (INT, [P, ctypes.POINTER(RdmEvalConfig), ctypes.POINTER(nat.RdActionNoise), P, P, P]),
    "rdm_evaluate_faulty": (INT, [P, ctypes.POINTER(RdmEvalConfig), ctypes.POINTER(nat.RdObsFaults),
                                  ctypes.POINTER(nat.RdActionNoise), P, P, P]),
    "rdm_set_teacher": (INT, [P, P, P, P]),
    "rdm_evaluate": (INT, [P, ctypes.POINTER(RdmEvalConfig), P, P, P]),
    "rdm_param_count": (INT, []),
    "rdm_create": (INT, [ctypes.POINTER(P), ctypes.POINTER(RdmConfig), INT, P]),
    "rdm_create_dtype": (INT, [ctypes.POINTER(P), ctypes.POINTER(RdmConfig), I32, INT, P]),
    "rdm_destroy": (INT, [P]),
    "rdm_set_stream": (INT, [P, P]),
    "rdm_set_params": (INT, [P, P]),
    "rdm_get_params": (INT, [P, P]),
    "rdm_reset": (INT, [P]),
    "rdm_forward": (INT, [P, P, I64, P]),
    "rdm_rollout": (INT, [P, P, P, I64, I64]),
    "rdm_apply": (INT, [P]),
    "rdm_step": (INT, [P, P, P, I64]),
    "rdm_grad_buffer": (P, [P]),
    "rdm_bind_grad_buffer": (INT, [P, P]),
    "rdm_get_counter": (INT, [P, ctypes.POINTER(I64)]),
    "rdm_read_metrics": (INT, [P, I64, P]),
})


def glorot_init(seed: int = 2) -> np.ndarray:
    """tf.layers.dense defaults: glorot_uniform kernels, zero biases (flat f32 [24,380])."""
    rng = np.random.RandomState(seed)
    out = []
    for a, b in zip(DIMS[:-1], DIMS[1:]):
        lim = math.sqrt(6.0 / (a + b))
        out.append(rng.uniform(-lim, lim, a * b).astype(np.float32))
        out.append(np.zeros(b, np.float32))
    return np.concatenate(out)


def rows(ob, prev_pdflat, prev_rew) -> torch.Tensor:
    """[..., 11] | [..., 4] | [..., 1] -> contiguous [n, 16] rows (mlp_train.py:52)."""
    x = torch.cat([ob, prev_pdflat, prev_rew], dim=-1).to(torch.float32)
    return x.reshape(-1, IN_DIM).contiguous()


@dataclass
class EnvsResult:
    """The buffers one act_envs / rollout_envs / step_envs call filled, step-major: entry [k, i] is
    env i's k-th step of the call.  They are the trainer's own (attach_envs), rewritten by the next
    call: clone to keep."""
    x: torch.Tensor          # [K, n, 16] the undropped rows ob | prev t_pdflat | prev reward
    t_pdflat: torch.Tensor   # [K, n, 4] the teacher's mean | logstd
    s_pdflat: torch.Tensor   # [K, n, 4] the student's (0 when the teacher stepped)
    reward: torch.Tensor     # [K, n]


@dataclass
class StudentMlpConfig:
    loss: str = "kl"            # mlp_train.py:71 (kl_loss); "mse" = action-MSE
    lr: float = 1e-4            # mlp_train.py:75-78
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    keep_prob: float = 1.0      # reference trains with KEEP_PROB = 0.5 (config.py:30)
    seed: int = 0               # dropout key
    init_seed: int = 2
    grid: int = 0
    metrics_len: int = 4096
    dtype: str = "f32"          # "bf16": layers 1-3 on the bf16 matrix path, f32 master and sums
                                # (reacher_student_mlp.h "Arithmetic"), in every call of the trainer

    def __post_init__(self):
        if self.dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {self.dtype!r}")

    def native(self, row_base: int = 0):
        """(rdm_config, RDM_DTYPE_*): what rdm_create_dtype takes."""
        if self.dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {self.dtype!r}")
        c = RdmConfig(loss=LOSSES[self.loss], lr=self.lr, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                      grid=self.grid, metrics_len=self.metrics_len, keep_prob=self.keep_prob,
                      seed=self.seed % 2 ** 64, row_base=int(row_base))
        return c, DTYPES[self.dtype]


class StudentMlpTrainer(EnvsActing):
    _ABI = "rdm"

    def __init__(self, cfg: StudentMlpConfig | None = None, device="cuda:0", rank: int = 0, world_size: int = 1,
                 process_group=None, params=None, row_base: int = 0):
        self.cfg = cfg or StudentMlpConfig()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("StudentMlpTrainer runs on a GPU (HIP) device only; there is no CPU path")
        self.rank, self.world, self.pg = rank, world_size, process_group
        c, dtype = self.cfg.native(row_base)   # a bad dtype raises before any native call
        self._lib = nat.load()
        assert self._lib.rdm_param_count() == N_PARAMS
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rdm_create_dtype(ctypes.byref(h), ctypes.byref(c), dtype, self.device.index or 0,
                                                 nat.stream_handle(self.device)), "rdm_create_dtype")
        self._h = h
        self.teacher = None   # the teacher of evaluate() and of the envs (set_teacher)
        self.n_envs, self.accum_steps, self._envs = 0, 0, None   # attach_envs
        self._init_acting()
        self._flags = None   # stepped_with
        self._grad = torch.zeros(N_PARAMS, dtype=torch.float32, device=self.device)
        nat.check(self._lib.rdm_bind_grad_buffer(self._h, nat.ptr(self._grad)), "rdm_bind_grad_buffer")
        self.set_params(glorot_init(self.cfg.init_seed) if params is None else params)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rdm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return nat.stream_handle(self.device)

    def _sync_stream(self):
        nat.check(self._lib.rdm_set_stream(self._h, self._stream()), "rdm_set_stream")

    # -- parameters ------------------------------------------------------------------
    def set_params(self, params):
        p = torch.as_tensor(np.asarray(params, np.float32) if not torch.is_tensor(params) else params,
                            dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        if p.numel() != N_PARAMS:
            raise ValueError(f"expected {N_PARAMS} parameters, got {p.numel()}")
        self._sync_stream()
        nat.check(self._lib.rdm_set_params(self._h, nat.ptr(p)), "rdm_set_params")
        torch.cuda.current_stream(self.device).synchronize()

    def params(self) -> torch.Tensor:
        out = torch.empty(N_PARAMS, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdm_get_params(self._h, nat.ptr(out)), "rdm_get_params")
        return out

    def set_teacher(self, p):
        """The teacher of evaluate(): an MlpPolicyParams (the 2x64 MlpPolicy with its observation
        filter), as DistillTrainer.set_teacher takes it."""
        f, mu, sd = p.device_tensors(self.device)
        self._sync_stream()
        nat.check(self._lib.rdm_set_teacher(self._h, nat.ptr(f), nat.ptr(mu), nat.ptr(sd)), "rdm_set_teacher")
        torch.cuda.current_stream(self.device).synchronize()
        self.teacher = p

    def reset_optimizer(self):
        self._sync_stream()
        nat.check(self._lib.rdm_reset(self._h), "rdm_reset")

    # -- compute -----------------------------------------------------------------------
    def _rows(self, x):
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device).reshape(-1, IN_DIM).contiguous()
        if x.shape[0] == 0:
            raise ValueError("empty batch")
        return x

    def forward(self, x) -> torch.Tensor:
        """s_pdflat [n, 4] of rows x [n, 16] (dropout off, as the reference's queries)."""
        x = self._rows(x)
        out = torch.empty(x.shape[0], PDFLAT_SHAPE, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdm_forward(self._h, nat.ptr(x), x.shape[0], nat.ptr(out)), "rdm_forward")
        return out

    def evaluate(self, n_envs: int = 4096, episodes: int = 1, *, seed: int = 0, env_base: int = 0,
                 first_episode: int = 0, draws=None, final_dist: bool = False, records: bool = False,
                 grid: int = 0, noise: str = "none", noise_scale: float = 1.0,
                 noise_seed: int | None = None, faults=None) -> EvalResult:
        """Roll ``n_envs`` evaluation envs through ``episodes`` consecutive 50-step episodes stepped
        with this student's mean action in ONE launch (rdm_evaluate): the phase-2 loop of
        mlp_train.train(student="mlp") without the optimiser steps.  Per step the teacher set by
        set_teacher() labels the observation, the student sees the row ob | the teacher's previous
        pdflat | the previous record's reward (zeros at an episode's first step; the reward is
        carried over resets, DeviceDataset.current_prev), and its unclipped mean steps the env.
        Bitwise the stepwise loop -- BatchedReacher.reset(), then 50 x {DistillTrainer.forward
        (teacher), rows(), forward(), BatchedReacher.step(mean)} per episode -- with no side effect
        on the trainer.  Episode e of env i resets from ``draws[e, i]`` ([E, n_envs, 6]: q0 q1 v0 v1
        tx ty) or, without a table, from Philox(seed, env_base + i, first_episode + e).  Returns a
        distill.EvalResult: returns [E, n]; final_dist [E, n]; records [E, n, 50, 21] in the dataset's
        layout (both pdflats, stepped_with = 1), so that records.view(E * n, 50, 21) goes into
        DeviceDataset.write_episodes.  Asynchronous on the current stream; no workspace: capturable.
        ``noise`` = "policy" or "fixed" (rdm_evaluate_noisy; action_noise.py): the student's action is
        perturbed, a = mean + noise_scale (exp(logstd) | 1) xi with xi keyed (noise_seed, env_base + i,
        first_episode + e, step) -- the return under perturbed actions, bitwise the stepwise loop with
        action_noise.perturb_actions before the step.  ``noise_seed`` defaults to ``seed``.  The envs'
        set_action_noise is never read here: the default is the noiseless return.
        ``faults`` = ("dropout" | "missing", keep_prob[, seed]) or a dict of them (rdm_evaluate_faulty;
        obs_faults.py): the student reads its observation through that mask, keyed (seed, env_base + i,
        first_episode + e, step, component) with the seed defaulting to ``seed``; the teacher and the
        records keep the clean observation.  Composes with ``noise``.  Bitwise the stepwise loop with
        obs_faults.mask_obs before the student's forward.  The envs' set_obs_faults is never read here."""
        nz = an.native(noise, noise_scale, seed if noise_seed is None else noise_seed)
        of = obf.parse(faults, seed)
        n, E = int(n_envs), int(episodes)
        if n < 1 or E < 1:
            raise ValueError("n_envs >= 1 and episodes >= 1")
        if self.teacher is None:
            raise RuntimeError("evaluate() needs a teacher: call set_teacher(MlpPolicyParams) first")
        table = None
        if draws is not None:
            table = torch.as_tensor(draws).to(self.device, torch.float32).contiguous()
            if table.shape != (E, n, 6):
                raise ValueError(f"draws must be [{E}, {n}, 6]")
        kw = dict(dtype=torch.float32, device=self.device)
        res = EvalResult(torch.empty(E, n, **kw),
                         torch.empty(E, n, **kw) if final_dist else None,
                         torch.empty(E, n, 50, 21, **kw) if records else None)
        c = RdmEvalConfig(n_envs=n, env_base=int(env_base), seed=int(seed) % 2 ** 64, episodes=E,
                          first_episode=int(first_episode), grid=int(grid),
                          draws=table.data_ptr() if table is not None else None)
        self._sync_stream()
        out = (nat.ptr(res.returns), nat.ptr(res.final_dist) if final_dist else None,
               nat.ptr(res.records) if records else None)
        if of is not None:
            nat.check(self._lib.rdm_evaluate_faulty(self._h, ctypes.byref(c), ctypes.byref(of),
                                                    None if noise == "none" else ctypes.byref(nz), *out),
                      "rdm_evaluate_faulty")
        elif noise == "none":
            nat.check(self._lib.rdm_evaluate(self._h, ctypes.byref(c), *out), "rdm_evaluate")
        else:
            nat.check(self._lib.rdm_evaluate_noisy(self._h, ctypes.byref(c), ctypes.byref(nz), *out),
                      "rdm_evaluate_noisy")
        self._keep_eval = table   # the launch reads it asynchronously
        return res

    # -- persistent envs: batched on-policy distillation --------------------------------------
    def attach_envs(self, n_envs: int, *, seed: int = 0, env_base: int = 0, grid: int = 0, accum_steps: int = 1,
                    flags: bool = False, actions: bool = False):
        """Give the trainer ``n_envs`` persistent lockstep envs (rdm_envs_attach; Philox resets keyed
        (seed, env_base + i, episode)) at episode 0, and allocate once the buffers every
        act_envs / rollout_envs / step_envs call fills: ``accum_steps`` = K env steps per call, so K n
        rows per optimiser step.  K = 50 puts all 50 episode phases of the lockstep envs into every
        batch.  Attaching again replaces the envs.  ``flags``: also allocate and bind ``stepped_with``
        (it is there anyway once a teacher share > 0 is set, and stays once made).  ``actions``: also
        allocate and bind ``actions``, the action that stepped each env (stays once made).  Single GPU
        only."""
        n, K = int(n_envs), int(accum_steps)
        if n < 1 or K < 1:
            raise ValueError("n_envs >= 1 and accum_steps >= 1")
        if self.world != 1:
            raise RuntimeError("the persistent envs are single-GPU (no rank-sharded variant)")
        c = RdmEnvsConfig(n_envs=n, env_base=int(env_base), seed=int(seed) % 2 ** 64, grid=int(grid))
        self._envs = None   # the handle's old envs go first
        self._sync_stream()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rdm_envs_attach(self._h, ctypes.byref(c)), "rdm_envs_attach")
        kw = dict(dtype=torch.float32, device=self.device)
        self._envs = EnvsResult(torch.zeros(K, n, IN_DIM, **kw), torch.zeros(K, n, PDFLAT_SHAPE, **kw),
                                torch.zeros(K, n, PDFLAT_SHAPE, **kw), torch.zeros(K, n, **kw))
        self.n_envs, self.accum_steps = n, K
        self._attach_acting(seed, K, n, actions)
        if flags or self._flags is not None or self.teacher_share > 0:
            self._bind_flags()

    # -- how the envs calls act: EnvsActing's settings, and what each leaves unchanged here ---------
    def set_action_noise(self, mode: str = "none", scale: float = 1.0, seed: int | None = None):
        """EnvsActing.set_action_noise.  Only the action changes: x, both pdflats, stepped_with and the
        training on every row are as without noise."""
        EnvsActing.set_action_noise(self, mode, scale, seed)

    def set_obs_faults(self, mode: str = "none", keep_prob: float = 1.0, seed: int | None = None):
        """EnvsActing.set_obs_faults, on the observation of the step (component k of env i's observation at
        (episode, step)).  x and both pdflats' buffers, stepped_with, actions and the training on every row
        are as without faults."""
        EnvsActing.set_obs_faults(self, mode, keep_prob, seed)

    def set_teacher_share(self, beta: float, seed: int | None = None):
        """EnvsActing.set_teacher_share.  The first beta > 0 allocates ``stepped_with``."""
        EnvsActing.set_teacher_share(self, beta, seed)
        if float(beta) > 0 and self._flags is None and self._envs is not None:
            self._bind_flags()

    def _bind_flags(self):
        self._flags = torch.ones(self.accum_steps, self.n_envs, dtype=torch.float32, device=self.device)
        nat.check(self._lib.rdm_envs_bind_stepped_with(self._h, nat.ptr(self._flags), self._flags.numel()),
                  "rdm_envs_bind_stepped_with")

    @property
    def stepped_with(self):
        """[accum_steps, n] f32, the trainer's own and rewritten by every envs call: 1 where the
        student's action stepped env i at the call's k-th step, 0 where the teacher's did (all 0 after a
        "teacher" call); rows past a shorter call's ``steps`` keep their old values.  None until a
        teacher share > 0 is set or attach_envs(..., flags=True) asks for it."""
        return self._flags

    def reset_envs(self):
        """Every env back to its episode 0; clocks, carried reward and previous fields to 0."""
        self._need_envs()
        self._sync_stream()
        nat.check(self._lib.rdm_envs_reset(self._h), "rdm_envs_reset")

    def _need_envs(self):
        if self._envs is None:
            raise RuntimeError("no envs attached: call attach_envs(n_envs) first")

    def _envs_call(self, name: str, act_with: str, steps) -> EnvsResult:
        self._need_envs()
        K = self.accum_steps if steps is None else int(steps)
        if not 1 <= K <= self.accum_steps:
            raise ValueError(f"steps must be 1 .. accum_steps = {self.accum_steps}, got {K}")
        if act_with not in ACT_WITH:
            raise ValueError(f"act_with must be 'teacher' or 'student', got {act_with!r}")
        if self.teacher is None:
            raise RuntimeError(f"{name} needs a teacher: call set_teacher(MlpPolicyParams) first")
        b = self._envs
        r = b if K == self.accum_steps else EnvsResult(b.x[:K], b.t_pdflat[:K], b.s_pdflat[:K], b.reward[:K])
        self._sync_stream()
        nat.check(getattr(self._lib, name)(self._h, ACT_WITH[act_with], K, nat.ptr(r.x), nat.ptr(r.t_pdflat),
                                           nat.ptr(r.s_pdflat), nat.ptr(r.reward)), name)
        return r

    def act_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """K = ``steps`` (default, and at most, ``accum_steps``) env steps of every env in ONE launch
        (rdm_envs_act), no training and no side effect on the parameters, Adam state, gradient or
        metrics; the result's tensors are the first K steps of the trainer's buffers.  Per step the teacher labels the
        observation, the row ob | the teacher's previous pdflat | the previous record's reward field is
        assembled (zeros at an episode's step 0), and the env is stepped with the student's mean on
        that row (``"student"``) or with the teacher's (``"teacher"``: the student is not evaluated,
        s_pdflat is 0).  Envs reset themselves after their step 49.  Bitwise the stepwise loop
        {DistillTrainer.forward (teacher), rows(), forward(), BatchedReacher.step(mean)}.  Asynchronous
        on the current stream, capturable; the device keeps the clock, so a replay takes the NEXT steps."""
        return self._envs_call("rdm_envs_act", act_with, steps)

    def rollout_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """act_envs, then the training launch on the K n rows it wrote: their gradient in grad()."""
        return self._envs_call("rdm_rollout_envs", act_with, steps)

    def step_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """act_envs, then one optimiser step on the K n rows it wrote: the parameters, gradient,
        metrics and counter of step(x, t_pdflat) on them (input dropout ``keep_prob`` included)."""
        return self._envs_call("rdm_step_envs", act_with, steps)

    def env_state(self):
        """(state [8, n] as BatchedReacher.get_state, env 0's step of the episode, its episode)."""
        self._need_envs()
        st = torch.empty(8, self.n_envs, dtype=torch.float32, device=self.device)
        s, e = ctypes.c_int32(), ctypes.c_int32()
        self._sync_stream()
        nat.check(self._lib.rdm_envs_get_state(self._h, nat.ptr(st), ctypes.byref(s), ctypes.byref(e)),
                  "rdm_envs_get_state")
        return st, s.value, e.value

    def rollout(self, x, t_pdflat, n_global: int | None = None) -> torch.Tensor:
        """Gradient of this rank's rows into grad(); returns the gradient tensor."""
        x = self._rows(x)
        t = torch.as_tensor(t_pdflat, dtype=torch.float32, device=self.device).reshape(-1, PDFLAT_SHAPE).contiguous()
        if t.shape[0] != x.shape[0]:
            raise ValueError("x and t_pdflat row counts differ")
        self._sync_stream()
        nat.check(self._lib.rdm_rollout(self._h, nat.ptr(x), nat.ptr(t), x.shape[0],
                                        int(n_global or x.shape[0])), "rdm_rollout")
        self._keep = (x, t)   # kernels are asynchronous: keep the inputs alive
        return self._grad

    def apply(self):
        self._sync_stream()
        nat.check(self._lib.rdm_apply(self._h), "rdm_apply")

    def step(self, x, t_pdflat, n_global: int | None = None):
        """sess.run([loss, minimize_adam]) (mlp_train.py:145-160): one optimiser step."""
        if self.world == 1:
            x = self._rows(x)
            t = torch.as_tensor(t_pdflat, dtype=torch.float32,
                                device=self.device).reshape(-1, PDFLAT_SHAPE).contiguous()
            if t.shape[0] != x.shape[0]:
                raise ValueError("x and t_pdflat row counts differ")
            self._sync_stream()
            nat.check(self._lib.rdm_step(self._h, nat.ptr(x), nat.ptr(t), x.shape[0]), "rdm_step")
            self._keep = (x, t)
            return
        self.rollout(x, t_pdflat, n_global)
        allreduce_sum_(self._grad, self.pg)
        self.apply()

    def graph_step(self, n: int):
        """One training step (rdm_step) on n rows captured into a HIP graph: returns
        step(x, t_pdflat), which copies into the graph's static buffers and replays."""
        if self.world != 1:
            raise RuntimeError("graph capture is for the single-rank step")
        x = torch.zeros(int(n), IN_DIM, device=self.device)
        t = torch.zeros(int(n), PDFLAT_SHAPE, device=self.device)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self._sync_stream()
            nat.check(self._lib.rdm_step(self._h, nat.ptr(x), nat.ptr(t), int(n)), "rdm_step")
        self._sync_stream()

        def step(xv, tv):
            x.copy_(torch.as_tensor(xv, dtype=torch.float32).reshape(x.shape))
            t.copy_(torch.as_tensor(tv, dtype=torch.float32).reshape(t.shape))
            g.replay()

        step.graph, step.inputs = g, (x, t)
        return step

    def grad(self) -> torch.Tensor:
        return self._grad

    def counter(self) -> int:
        v = ctypes.c_int64()
        nat.check(self._lib.rdm_get_counter(self._h, ctypes.byref(v)), "rdm_get_counter")
        return v.value

    def metrics(self, count: int = 1) -> np.ndarray:
        """[count, 4]: loss, sum |mu_s - mu_t|^2, rows, 0 of the last optimiser steps."""
        out = np.zeros((count, 4), np.float64)
        nat.check(self._lib.rdm_read_metrics(self._h, count, out.ctypes.data_as(ctypes.c_void_p)),
                  "rdm_read_metrics")
        return out
