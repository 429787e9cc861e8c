"""Host layer of the reference's LSTM student (include/reacher_student_lstm.h).

``StudentLstmTrainer`` is the 'LSTM' scope of the reference's lstm_train.py (:35-79): the
graph ``student_lstm_graph`` (student_nn.py:21-49: dense prev-pdflat embedding, TF1
LSTMCell(200), a 200-64-128-64-32-4 head per unrolled step), ``kl_loss`` (loss.py:3-13) and TF1 Adam, run by
csrc/student_lstm.hip.  Tensors are the reference's window layout: ob [T, B, 11],
prev_pdflat [T, B, 4], t_pdflat / pdflat [T, B, 4], state [2, B, 200] = (c, m).

``StudentLstmConfig(dtype="bf16")`` (rdl_create_dtype) runs the three products of the cell matrix on
the bf16 MFMAs in forward / rollout / step and the training pass of rollout_envs / step_envs, with
f32 master weights, heads and sums; the checkpoint is the f32 master plus slots either way.  The
closed-loop query of evaluate, act_envs and the act phase of rollout_envs / step_envs has its own
setting, ``query_dtype`` (rdl_set_query_dtype): "f32" (default) keeps it on the f32 master weights,
"bf16" (bf16 trainers only) runs it on the same bf16 cell as forward, so that one query step is
bitwise one forward on the env's window and the student that acts is the student that is trained.

Multi-GPU: windows sharded contiguously (row_base = first global window), one
all_reduce(SUM) of the flat gradient (511,880 floats at T = 10: the shared cell and one
head per unrolled step) per optimiser step.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from . import action_noise as an
from . import obs_faults as obf
from ._envs_acting import EnvsActing
from .config import LSTM_BATCH_SIZE, NUM_UNITS, OBSPACE_SHAPE, PDFLAT_SHAPE, STEPS_UNROLLED
from .dist import allreduce_sum_
from .distill import EvalResult

P = nat.P
I32, I64, U64, F32, INT = nat.I32, nat.I64, nat.U64, nat.F32, nat.INT

HEAD = (NUM_UNITS, 64, 128, 64, 32, 4)
CELL_SHAPES = [("Wp", (4, 32)), ("bp", (32,)), ("Wl", (OBSPACE_SHAPE + 32 + NUM_UNITS, 4 * NUM_UNITS)),
               ("bl", (4 * NUM_UNITS,))]
HEAD_SHAPES = [x for k, (a, b) in enumerate(zip(HEAD[:-1], HEAD[1:]))
               for x in ((f"W{k + 1}", (a, b)), (f"b{k + 1}", (b,)))]


def shapes(T: int = STEPS_UNROLLED):
    """The flat layout in variable-creation order: the shared prev-pdflat dense and LSTMCell, then
    one head per unrolled step (the reference's tf.layers.dense calls inside its loop over the T
    steps create new variables at every step, student_nn.py:40-47; TF names dense_1..dense_5T)."""
    return CELL_SHAPES + [(f"h{t}/{n}", s) for t in range(T) for n, s in HEAD_SHAPES]


def n_params(T: int = STEPS_UNROLLED) -> int:
    return sum(int(np.prod(s)) for _, s in shapes(T))


N_PARAMS = n_params(STEPS_UNROLLED)   # 511,880 at the reference's T = 10
LOSSES = {"mse": 0, "kl": 1}
DTYPES = {"f32": 0, "bf16": 1}            # RDL_DTYPE_*


class RdlConfig(ctypes.Structure):
    _fields_ = [("loss", I32), ("lr", F32), ("beta1", F32), ("beta2", F32), ("eps", F32), ("steps", I32),
                ("max_windows", I32), ("metrics_len", I32), ("keep_prob", F32), ("seed", U64), ("row_base", I64),
                ("kernels", I32)]


class RdlEvalConfig(ctypes.Structure):
    _fields_ = [("n_envs", I64), ("env_base", I64), ("seed", U64), ("episodes", I32), ("first_episode", I32),
                ("grid", I32), ("draws", P)]


class RdlEnvsConfig(ctypes.Structure):
    _fields_ = [("n_envs", I64), ("env_base", I64), ("seed", U64), ("grid", I32)]


ACT_WITH = {"teacher": 0, "student": 1}   # RDL_ACT_*
_ENVS_TRAIN = (INT, [P, INT, INT, P, P, P, P, P])

nat.register({
    "rdl_envs_attach": (INT, [P, ctypes.POINTER(RdlEnvsConfig)]),
    "rdl_envs_reset": (INT, [P]),
    "rdl_envs_act": (INT, [P, INT, INT, P, P, P, P, P, I64]),
    "rdl_rollout_envs": _ENVS_TRAIN,
    "rdl_step_envs": _ENVS_TRAIN,
    "rdl_envs_get_state": (INT, [P, P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
    "rdl_envs_get_query_state": (INT, [P, P]),
    **nat.envs_acting("rdl"),
    "rdl_evaluate_faulty": (INT, [P, ctypes.POINTER(RdlEvalConfig), ctypes.POINTER(nat.RdObsFaults),
                                  ctypes.POINTER(nat.RdActionNoise), P, P, P, P, P]),
    "rdl_evaluate_noisy": (INT, [P, ctypes.POINTER(RdlEvalConfig), ctypes.POINTER(nat.RdActionNoise), P, P, P, P, P]),
    "rdl_set_teacher": (INT, [P, P, P, P]),
    "rdl_evaluate": (INT, [P, ctypes.POINTER(RdlEvalConfig), P, P, P, P, P]),
    "rdl_param_count": (I64, [I32]),
    "rdl_create": (INT, [ctypes.POINTER(P), ctypes.POINTER(RdlConfig), INT, P]),
    "rdl_create_dtype": (INT, [ctypes.POINTER(P), ctypes.POINTER(RdlConfig), I32, INT, P]),
    "rdl_set_query_dtype": (INT, [P, I32]),
    "rdl_query_dtype": (INT, [P]),
    "rdl_destroy": (INT, [P]),
    "rdl_set_stream": (INT, [P, P]),
    "rdl_set_params": (INT, [P, P]),
    "rdl_get_params": (INT, [P, P]),
    "rdl_reset": (INT, [P]),
    "rdl_forward": (INT, [P, P, P, P, I64, P, P]),
    "rdl_rollout": (INT, [P, P, P, P, P, I64, I64]),
    "rdl_apply": (INT, [P]),
    "rdl_step": (INT, [P, P, P, P, P, I64]),
    "rdl_grad_buffer": (P, [P]),
    "rdl_bind_grad_buffer": (INT, [P, P]),
    "rdl_get_counter": (INT, [P, ctypes.POINTER(I64)]),
    "rdl_read_metrics": (INT, [P, I64, P]),
    "rdl_final_state": (INT, [P, I64, P]),
    "rdl_get_slots": (INT, [P, P, P]),
    "rdl_set_slots": (INT, [P, P, P]),
    "rdl_head_path": (INT, [P]),
})


def glorot_init(seed: int = 3, T: int = STEPS_UNROLLED) -> np.ndarray:
    """glorot_uniform kernels (tf.layers.dense and LSTMCell defaults), zero biases."""
    rng = np.random.RandomState(seed)
    out = []
    for _, s in shapes(T):
        if len(s) == 2:
            lim = math.sqrt(6.0 / (s[0] + s[1]))
            out.append(rng.uniform(-lim, lim, s[0] * s[1]).astype(np.float32))
        else:
            out.append(np.zeros(s, np.float32))
    return np.concatenate(out)


@dataclass
class EnvsResult:
    """The buffers one act_envs / rollout_envs / step_envs call filled.  records and reward are
    step-major: entry [k, i] is env i's k-th step of the call.  The window tensors (None when the call
    wrote none) hold the query windows that lie wholly inside an episode, ordered by step, then by env.
    They are the trainer's own (attach_envs), rewritten by the next call: clone to keep."""
    records: torch.Tensor            # [K, n, 21] ob[11] | reward | t_pdflat[4] | s_pdflat[4] | stepped_with
    reward: torch.Tensor             # [K, n]
    ob_w: torch.Tensor | None        # [T, B, 11]
    prev_w: torch.Tensor | None      # [T, B, 4] the previous record's t_pdflat (0 at an episode's step 0)
    t_w: torch.Tensor | None         # [T, B, 4] the records' own t_pdflat


@dataclass
class StudentLstmConfig:
    loss: str = "kl"                  # lstm_train.py:71
    lr: float = 1e-3                  # lstm_train.py:74
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    steps: int = STEPS_UNROLLED       # T
    max_windows: int = LSTM_BATCH_SIZE
    keep_prob: float = 1.0            # reference trains with KEEP_PROB = 0.5
    seed: int = 0
    init_seed: int = 3
    metrics_len: int = 4096
    step_recurrence: bool = False     # force the per-step recurrence launches (else: persistent at <= 32 windows)
    layer_head: bool = False          # force the per-layer head GEMMs (else: one launch at <= 16,384 rows)
    dtype: str = "f32"                # "bf16": the cell matrix's three products (forward, data and weight
                                      # gradient) on the bf16 MFMAs in forward / rollout / step and the training
                                      # pass of the envs calls; f32 master, sums, heads; evaluate / act_envs stay
                                      # f32; always the per-step recurrence (step_recurrence has no effect)
    query_dtype: str = "f32"          # "bf16" (needs dtype="bf16"): the closed-loop query of evaluate / act_envs /
                                      # the act phase of rollout_envs / step_envs on the bf16 cell too: a query
                                      # step is bitwise one forward on the env's window

    def __post_init__(self):
        self.native_dtype()
        self.native_query_dtype()

    def native_dtype(self) -> int:
        """RDL_DTYPE_* of ``dtype``: what rdl_create_dtype takes."""
        if not isinstance(self.dtype, str) or self.dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {self.dtype!r}")
        return DTYPES[self.dtype]

    def native_query_dtype(self) -> int:
        """RDL_DTYPE_* of ``query_dtype``: what rdl_set_query_dtype takes."""
        return query_dtype_of(self.query_dtype, self.dtype)


def query_dtype_of(name, dtype: str) -> int:
    """RDL_DTYPE_* of the query dtype ``name`` on a trainer of ``dtype``; ValueError for an unknown name
    and for "bf16" on an f32 trainer (no bf16 image of Wl, and its training would not match the query)."""
    if not isinstance(name, str) or name not in DTYPES:
        raise ValueError(f"query_dtype must be one of {sorted(DTYPES)}, got {name!r}")
    if name == "bf16" and dtype != "bf16":
        raise ValueError(f'query_dtype="bf16" requires dtype="bf16", got dtype={dtype!r}')
    return DTYPES[name]


class StudentLstmTrainer(EnvsActing):
    _ABI = "rdl"

    def __init__(self, cfg: StudentLstmConfig | None = None, device="cuda:0", rank: int = 0, world_size: int = 1,
                 process_group=None, params=None, row_base: int = 0):
        self.cfg = cfg or StudentLstmConfig()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("StudentLstmTrainer runs on a GPU (HIP) device only; there is no CPU path")
        self.rank, self.world, self.pg = rank, world_size, process_group
        self.T = int(self.cfg.steps)
        dtype = self.cfg.native_dtype()   # a bad dtype raises before any native call
        qdtype = self.cfg.native_query_dtype()
        self._lib = nat.load()
        self.n_params = n_params(self.T)
        assert self._lib.rdl_param_count(self.T) == self.n_params
        c = RdlConfig(loss=LOSSES[self.cfg.loss], lr=self.cfg.lr, beta1=self.cfg.beta1, beta2=self.cfg.beta2,
                      eps=self.cfg.eps, steps=self.T, max_windows=int(self.cfg.max_windows),
                      metrics_len=self.cfg.metrics_len, keep_prob=self.cfg.keep_prob,
                      seed=self.cfg.seed % 2 ** 64, row_base=int(row_base),
                      kernels=int(bool(self.cfg.step_recurrence)) | 2 * int(bool(self.cfg.layer_head)))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rdl_create_dtype(ctypes.byref(h), ctypes.byref(c), dtype, self.device.index or 0,
                                                 nat.stream_handle(self.device)), "rdl_create_dtype")
        self._h = h
        nat.check(self._lib.rdl_set_query_dtype(self._h, qdtype), "rdl_set_query_dtype")
        self.teacher = None   # evaluate()'s teacher (set_teacher)
        self._envs = None     # attach_envs()'s buffers
        self._init_acting()
        self._grad = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        nat.check(self._lib.rdl_bind_grad_buffer(self._h, nat.ptr(self._grad)), "rdl_bind_grad_buffer")
        self.set_params(glorot_init(self.cfg.init_seed, self.T) if params is None else params)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rdl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync_stream(self):
        nat.check(self._lib.rdl_set_stream(self._h, nat.stream_handle(self.device)), "rdl_set_stream")

    # -- parameters ------------------------------------------------------------------
    def set_params(self, params):
        p = (params if torch.is_tensor(params) else torch.from_numpy(np.asarray(params, np.float32)))
        p = p.to(self.device, torch.float32).reshape(-1).contiguous()
        if p.numel() != self.n_params:
            raise ValueError(f"expected {self.n_params} parameters, got {p.numel()}")
        self._sync_stream()
        nat.check(self._lib.rdl_set_params(self._h, nat.ptr(p)), "rdl_set_params")
        torch.cuda.current_stream(self.device).synchronize()

    def set_teacher(self, p):
        """The teacher of evaluate(): an MlpPolicyParams (the 2x64 MlpPolicy with its observation
        filter), as DistillTrainer.set_teacher takes it."""
        f, mu, sd = p.device_tensors(self.device)
        self._sync_stream()
        nat.check(self._lib.rdl_set_teacher(self._h, nat.ptr(f), nat.ptr(mu), nat.ptr(sd)), "rdl_set_teacher")
        torch.cuda.current_stream(self.device).synchronize()
        self.teacher = p

    def set_query_dtype(self, name: str):
        """The arithmetic of the closed-loop query (evaluate, act_envs, the act phase of rollout_envs /
        step_envs) from the next call on: "f32", the master weights, or "bf16" on a dtype="bf16" trainer,
        the bf16 cell of forward (rdl_set_query_dtype; host-only).  A refused name leaves the setting."""
        nat.check(self._lib.rdl_set_query_dtype(self._h, query_dtype_of(name, self.cfg.dtype)), "rdl_set_query_dtype")

    @property
    def query_dtype(self) -> str:
        """"f32" or "bf16": what the handle's closed-loop query runs in (rdl_query_dtype)."""
        r = self._lib.rdl_query_dtype(self._h)
        if r < 0:
            raise RuntimeError("query_dtype: the trainer is closed")
        return next(k for k, v in DTYPES.items() if v == r)

    @property
    def fused_head(self) -> bool:
        """True if batches of at most 16,384 rows run the fused head kernels (rdl_head_path)."""
        r = self._lib.rdl_head_path(self._h)
        if r < 0:
            nat.check(r, "rdl_head_path")
        return r == 1

    def params(self) -> torch.Tensor:
        out = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdl_get_params(self._h, nat.ptr(out)), "rdl_get_params")
        return out

    def _slots(self):
        m = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        v = torch.empty_like(m)
        self._sync_stream()
        nat.check(self._lib.rdl_get_slots(self._h, nat.ptr(m), nat.ptr(v)), "rdl_get_slots")
        torch.cuda.current_stream(self.device).synchronize()
        return m, v

    def save(self, path: str):
        """tf.train.Saver(var_list=LSTM/*).save (reference lstm_train.py:86-87,199): the
        parameters and the Adam slots m, v.  A path ending in '.safetensors' is written as one
        safetensors file; any other path is a TF checkpoint prefix (``path.index`` +
        ``path.data-00000-of-00001``, the reference's own format and variable names,
        tf_checkpoint.save_lstm).  Nothing executable either way."""
        m, v = self._slots()
        p = self.params()
        if path.endswith(".safetensors"):
            from safetensors.torch import save_file
            save_file({"params": p.cpu(), "adam_m": m.cpu(), "adam_v": v.cpu()}, path)
        else:
            from . import tf_checkpoint
            tf_checkpoint.save_lstm(path, p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), self.T)

    @staticmethod
    def checkpoint_exists(path: str) -> bool:
        from . import tf_checkpoint
        return os.path.exists(path) if path.endswith(".safetensors") else tf_checkpoint.exists(path)

    def load(self, path: str):
        """saver.restore (reference lstm_train.py:102-107): parameters and Adam slots from
        `path` (format by suffix, as save); the beta powers and step counter start afresh, as
        the reference initialises the Adam variables before restoring the 'LSTM' scope
        (:99-105).  A TF checkpoint without Adam slots restores the parameters and zero slots."""
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            d = load_file(path)
            p, m, v = d["params"], d["adam_m"], d["adam_v"]
        else:
            from . import tf_checkpoint
            p, m, v = tf_checkpoint.load_lstm(path, self.T)
            p = torch.from_numpy(p)
            m = torch.zeros_like(p) if m is None else torch.from_numpy(m)
            v = torch.zeros_like(p) if v is None else torch.from_numpy(v)
        if p.numel() != self.n_params:
            raise ValueError(f"{path}: {p.numel()} parameters, expected {self.n_params}")
        self.reset_optimizer()
        self.set_params(p)
        m = m.to(self.device, torch.float32).contiguous()
        v = v.to(self.device, torch.float32).contiguous()
        self._sync_stream()
        nat.check(self._lib.rdl_set_slots(self._h, nat.ptr(m), nat.ptr(v)), "rdl_set_slots")
        torch.cuda.current_stream(self.device).synchronize()

    def reset_optimizer(self):
        self._sync_stream()
        nat.check(self._lib.rdl_reset(self._h), "rdl_reset")

    # -- compute -----------------------------------------------------------------------
    def _t(self, x, last):
        x = torch.as_tensor(x, dtype=torch.float32, device=self.device).contiguous()
        if x.dim() != 3 or x.shape[0] != self.T or x.shape[2] != last:
            raise ValueError(f"expected [T={self.T}, B, {last}], got {tuple(x.shape)}")
        return x

    def _windows(self, ob, prev, tgt=None, state0=None):
        ob, prev = self._t(ob, OBSPACE_SHAPE), self._t(prev, PDFLAT_SHAPE)
        B = ob.shape[1]
        if B == 0 or prev.shape[1] != B or B > self.cfg.max_windows:
            raise ValueError(f"bad window count {B} (max_windows {self.cfg.max_windows})")
        if tgt is not None:
            tgt = self._t(tgt, PDFLAT_SHAPE)
            if tgt.shape[1] != B:
                raise ValueError("t_pdflat window count differs")
        if state0 is not None:
            state0 = torch.as_tensor(state0, dtype=torch.float32, device=self.device).contiguous()
            if tuple(state0.shape) != (2, B, NUM_UNITS):
                raise ValueError(f"state must be [2, {B}, {NUM_UNITS}]")
        return ob, prev, tgt, state0, B

    def forward(self, ob, prev_pdflat, state0=None):
        """(pdflat [T, B, 4], final state [2, B, 200]) with dropout off (lstm_train.py:171-183)."""
        ob, prev, _, st, B = self._windows(ob, prev_pdflat, None, state0)
        out = torch.empty(self.T, B, PDFLAT_SHAPE, dtype=torch.float32, device=self.device)
        fin = torch.empty(2, B, NUM_UNITS, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdl_forward(self._h, nat.ptr(ob), nat.ptr(prev), nat.ptr(st) if st is not None else None,
                                        B, nat.ptr(out), nat.ptr(fin)), "rdl_forward")
        return out, fin

    def evaluate(self, n_envs: int = 4096, episodes: int = 1, *, seed: int = 0, env_base: int = 0,
                 first_episode: int = 0, draws=None, state0=None, final_dist: bool = False, records: bool = False,
                 final_state: bool = False, grid: int = 0, noise: str = "none", noise_scale: float = 1.0,
                 noise_seed: int | None = None, faults=None) -> EvalResult:
        """Roll ``n_envs`` evaluation envs through ``episodes`` consecutive 50-step episodes stepped
        with this student's mean action in ONE rollout launch (rdl_evaluate): the query loop of
        lstm_train.train without the optimiser steps, each env being column B-1 of the driver's
        query.  Per step the teacher set by set_teacher() labels the observation; the student sees the
        window of the episode's last T records (ob | the teacher's previous pdflat; zero rows before
        the episode's first), runs from the final (c, h) of the env's previous query -- carried over
        episode boundaries, ``state0`` [2, n, 200] or zeros at the call's first step -- and the
        unclipped mean of unrolled position T-1 steps the env.  Bitwise the stepwise loop --
        BatchedReacher.reset(), then 50 x {DistillTrainer.forward (teacher), the windows,
        forward(ob_w, prev_w, state)[T-1], BatchedReacher.step(mean)} per episode -- with no side
        effect on the trainer (on a bf16 trainer: this trainer's loop under query_dtype="bf16", an f32
        trainer's with the same parameters under the default "f32").  Episode e of env i resets from ``draws[e, i]`` ([E, n_envs, 6]) or,
        without a table, from Philox(seed, env_base + i, first_episode + e).  Returns a
        distill.EvalResult: returns [E, n]; final_dist [E, n]; records [E, n, 50, 21] in the dataset's
        layout (stepped_with = 1); state [2, n, 200] = (c, h) after the last query with
        ``final_state``.  Asynchronous on the current stream; no allocation in the library: capturable.
        ``noise`` = "policy" or "fixed" (rdl_evaluate_noisy; action_noise.py): the student's action is
        perturbed, a = mean + noise_scale (exp(logstd) | 1) xi with xi keyed (noise_seed, env_base + i,
        first_episode + e, step) -- the return under perturbed actions, bitwise the stepwise loop with
        action_noise.perturb_actions before the step.  ``noise_seed`` defaults to ``seed``.  The envs'
        set_action_noise is never read here: the default is the noiseless return.
        ``faults`` = ("dropout" | "missing", keep_prob[, seed]) or a dict of them (rdl_evaluate_faulty;
        obs_faults.py): the student reads every record of its windows through that mask, record j of an
        episode keyed (seed, env_base + i, first_episode + e, j, component) wherever in a window it
        stands, the seed defaulting to ``seed``; the teacher and the records keep the clean observation.
        Composes with ``noise``.  Bitwise the stepwise loop with obs_faults.mask_obs on every record as it
        enters the window.  The envs' set_obs_faults is never read here."""
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
        if state0 is not None:
            state0 = torch.as_tensor(state0).to(self.device, torch.float32).contiguous()
            if tuple(state0.shape) != (2, n, NUM_UNITS):
                raise ValueError(f"state0 must be [2, {n}, {NUM_UNITS}]")
        kw = dict(dtype=torch.float32, device=self.device)
        res = EvalResult(torch.empty(E, n, **kw),
                         torch.empty(E, n, **kw) if final_dist else None,
                         torch.empty(E, n, 50, 21, **kw) if records else None,
                         torch.empty(2, n, NUM_UNITS, **kw) if final_state else None)
        c = RdlEvalConfig(n_envs=n, env_base=int(env_base), seed=int(seed) % 2 ** 64, episodes=E,
                          first_episode=int(first_episode), grid=int(grid),
                          draws=table.data_ptr() if table is not None else None)
        self._sync_stream()
        out = (nat.ptr(state0) if state0 is not None else None, nat.ptr(res.returns),
               nat.ptr(res.final_dist) if final_dist else None, nat.ptr(res.records) if records else None,
               nat.ptr(res.state) if final_state else None)
        if of is not None:
            nat.check(self._lib.rdl_evaluate_faulty(self._h, ctypes.byref(c), ctypes.byref(of),
                                                    None if noise == "none" else ctypes.byref(nz), *out),
                      "rdl_evaluate_faulty")
        elif noise == "none":
            nat.check(self._lib.rdl_evaluate(self._h, ctypes.byref(c), *out), "rdl_evaluate")
        else:
            nat.check(self._lib.rdl_evaluate_noisy(self._h, ctypes.byref(c), ctypes.byref(nz), *out),
                      "rdl_evaluate_noisy")
        self._keep_eval = (table, state0)   # the launch reads them asynchronously
        return res

    # -- persistent envs: batched on-policy distillation --------------------------------------
    def attach_envs(self, n_envs: int, *, seed: int = 0, env_base: int = 0, grid: int = 0, accum_steps: int = 50,
                    actions: bool = False):
        """Give the trainer ``n_envs`` persistent lockstep envs (rdl_envs_attach; Philox resets keyed
        (seed, env_base + i, episode)) at episode 0 with a zero query state, and allocate once the
        buffers every act_envs / rollout_envs / step_envs call fills: ``accum_steps`` = K env steps
        per call at the most.  A call of a multiple of 50 steps holds n (K / 50) (51 - T) training
        windows (any 50 consecutive lockstep steps hold 51 - T queries whose window lies inside one
        episode); ``max_windows`` of the config must cover that for the training calls.  Attaching
        again replaces the envs.  ``actions``: also allocate and bind ``actions``, the action that
        stepped each env (stays once made).  Single GPU only."""
        n, K = int(n_envs), int(accum_steps)
        if n < 1 or K < 1:
            raise ValueError("n_envs >= 1 and accum_steps >= 1")
        if self.world != 1:
            raise RuntimeError("the persistent envs are single-GPU (no rank-sharded variant)")
        c = RdlEnvsConfig(n_envs=n, env_base=int(env_base), seed=int(seed) % 2 ** 64, grid=int(grid))
        self._envs = None   # the handle's old envs go first
        self._sync_stream()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rdl_envs_attach(self._h, ctypes.byref(c)), "rdl_envs_attach")
        kw = dict(dtype=torch.float32, device=self.device)
        T = self.T
        Bm = n * (K // 50) * (51 - T) if T <= 50 else 0   # windows of the longest multiple-of-50 call
        self._envs = EnvsResult(torch.zeros(K, n, 21, **kw), torch.zeros(K, n, **kw),
                                torch.zeros(T * Bm * OBSPACE_SHAPE, **kw) if Bm else None,
                                torch.zeros(T * Bm * PDFLAT_SHAPE, **kw) if Bm else None,
                                torch.zeros(T * Bm * PDFLAT_SHAPE, **kw) if Bm else None)
        self.n_envs, self.accum_steps = n, K
        self._attach_acting(seed, K, n, actions)

    # -- how the envs calls act: EnvsActing's settings, and what each leaves unchanged here ---------
    def set_obs_faults(self, mode: str = "none", keep_prob: float = 1.0, seed: int | None = None):
        """EnvsActing.set_obs_faults, on the records of the window: component k of record j of env i's open
        episode is masked by (seed, env_base + i, episode, j, k) at every position of every window that
        holds the record -- a reading once lost stays lost.  Through the student's pdflat (c, h) changes
        too; the records and the windows (ob_w, prev_w, t_w) hold the clean readings."""
        EnvsActing.set_obs_faults(self, mode, keep_prob, seed)

    def set_action_noise(self, mode: str = "none", scale: float = 1.0, seed: int | None = None):
        """EnvsActing.set_action_noise.  Only the action changes: the records, (c, h), the ring, the
        windows and the training on every window are as without noise."""
        EnvsActing.set_action_noise(self, mode, scale, seed)

    def set_teacher_share(self, beta: float, seed: int | None = None):
        """EnvsActing.set_teacher_share.  A step the teacher's coin took writes 0 to the record's
        stepped_with; (c, h), the ring and the windows are the student call's."""
        EnvsActing.set_teacher_share(self, beta, seed)

    def reset_envs(self):
        """Every env back to its episode 0; clock, carried reward, query state and history to 0."""
        self._need_envs()
        self._sync_stream()
        nat.check(self._lib.rdl_envs_reset(self._h), "rdl_envs_reset")

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
        b, T = self._envs, self.T
        train = name != "rdl_envs_act"
        B = self.n_envs * (K // 50) * (51 - T) if K % 50 == 0 and T <= 50 else 0   # windows only for whole episodes' worth
        dims = (OBSPACE_SHAPE, PDFLAT_SHAPE, PDFLAT_SHAPE)
        if B:
            w = [x[:T * B * d].view(T, B, d) for x, d in zip((b.ob_w, b.prev_w, b.t_w), dims)]
        elif train:   # no whole episode's worth of steps: the library names what is wrong, given any buffers
            w = [torch.zeros(T, 1, d, dtype=torch.float32, device=self.device) for d in dims]
        else:
            w = [None, None, None]
        r = EnvsResult(b.records[:K], b.reward[:K], *(w if B else [None, None, None]))
        self._sync_stream()
        args = [self._h, ACT_WITH[act_with], K, nat.ptr(r.records), nat.ptr(r.reward)] + \
               [nat.ptr(x) if x is not None else None for x in w]
        if not train:
            args.append(B)
        nat.check(getattr(self._lib, name)(*args), name)
        return r

    def act_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """K = ``steps`` (default, and at most, ``accum_steps``) env steps of every env in ONE launch
        (rdl_envs_act), no training and no side effect on the parameters, Adam state, gradient, metrics
        or counter.  Per step the teacher labels the observation; under ``"student"`` the window of the
        episode's last T records (zero rows before its first) runs from the env's carried (c, h) and
        the mean of unrolled position T-1 steps the env; under ``"teacher"`` the teacher's mean does,
        the student is not evaluated, (c, h) stays, s_pdflat and stepped_with are 0.  Envs reset
        themselves after their step 49; (c, h) carries over.  The x rows of the carried records are
        re-formed with the parameters the call finds.  Bitwise the stepwise loop
        {DistillTrainer.forward (teacher), the window, forward(ob_w, prev_w, state)[T-1],
        BatchedReacher.step(mean)}.  The result's window tensors are filled when ``steps`` is a
        multiple of 50 (B = n (steps / 50) (51 - T)), else None.  Asynchronous on the current stream,
        capturable; the device keeps the clock, so a replay takes the NEXT steps."""
        return self._envs_call("rdl_envs_act", act_with, steps)

    def rollout_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """act_envs (``steps`` a multiple of 50), then the training pass on the windows it wrote, from
        a zero initial state: their gradient in grad()."""
        return self._envs_call("rdl_rollout_envs", act_with, steps)

    def step_envs(self, act_with: str = "student", steps: int | None = None) -> EnvsResult:
        """act_envs (``steps`` a multiple of 50), then one optimiser step on the windows it wrote: the
        parameters, gradient, metrics, counter and final_state of step(ob_w, prev_w, t_w) on them
        (input dropout ``keep_prob`` included)."""
        return self._envs_call("rdl_step_envs", act_with, steps)

    def env_state(self):
        """(state [8, n] as BatchedReacher.get_state, env 0's step of the episode, its episode)."""
        self._need_envs()
        st = torch.empty(8, self.n_envs, dtype=torch.float32, device=self.device)
        s, e = ctypes.c_int32(), ctypes.c_int32()
        self._sync_stream()
        nat.check(self._lib.rdl_envs_get_state(self._h, nat.ptr(st), ctypes.byref(s), ctypes.byref(e)),
                  "rdl_envs_get_state")
        return st, s.value, e.value

    def query_state(self) -> torch.Tensor:
        """[2, n, 200] = (c, h) of the envs after their last student query (zeros after attach / reset)."""
        self._need_envs()
        out = torch.empty(2, self.n_envs, NUM_UNITS, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdl_envs_get_query_state(self._h, nat.ptr(out)), "rdl_envs_get_query_state")
        return out

    def rollout(self, ob, prev_pdflat, t_pdflat, state0=None, windows_global: int | None = None):
        ob, prev, tgt, st, B = self._windows(ob, prev_pdflat, t_pdflat, state0)
        self._sync_stream()
        nat.check(self._lib.rdl_rollout(self._h, nat.ptr(ob), nat.ptr(prev), nat.ptr(tgt),
                                        nat.ptr(st) if st is not None else None, B, int(windows_global or B)),
                  "rdl_rollout")
        self._keep = (ob, prev, tgt, st)
        return self._grad

    def apply(self):
        self._sync_stream()
        nat.check(self._lib.rdl_apply(self._h), "rdl_apply")

    def step(self, ob, prev_pdflat, t_pdflat, state0=None, windows_global: int | None = None):
        """sess.run([loss, minimize_adam]) (lstm_train.py:145-160)."""
        if self.world == 1:
            ob, prev, tgt, st, B = self._windows(ob, prev_pdflat, t_pdflat, state0)
            self._sync_stream()
            nat.check(self._lib.rdl_step(self._h, nat.ptr(ob), nat.ptr(prev), nat.ptr(tgt),
                                         nat.ptr(st) if st is not None else None, B), "rdl_step")
            self._keep = (ob, prev, tgt, st)
            return
        self.rollout(ob, prev_pdflat, t_pdflat, state0, windows_global)
        allreduce_sum_(self._grad, self.pg)
        self.apply()

    def graph_step(self, windows: int):
        """One training step (rdl_step, zero initial state) for `windows` windows captured
        into a HIP graph: returns step(ob, prev_pdflat, t_pdflat), which copies the inputs
        into the graph's static buffers and replays (no host launches; the reference's
        20-window step is launch-bound).  Replays are the same computation as step()."""
        if self.world != 1:
            raise RuntimeError("graph capture is for the single-rank step")
        T, B = self.T, int(windows)
        if not 0 < B <= self.cfg.max_windows:
            raise ValueError(f"bad window count {B}")
        ob = torch.zeros(T, B, OBSPACE_SHAPE, device=self.device)
        prev = torch.zeros(T, B, PDFLAT_SHAPE, device=self.device)
        tgt = torch.zeros(T, B, PDFLAT_SHAPE, device=self.device)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        with torch.cuda.graph(g):
            self._sync_stream()
            nat.check(self._lib.rdl_step(self._h, nat.ptr(ob), nat.ptr(prev), nat.ptr(tgt), None, B), "rdl_step")
        self._sync_stream()

        def step(o, p, t):
            ob.copy_(torch.as_tensor(o, dtype=torch.float32).reshape(ob.shape))
            prev.copy_(torch.as_tensor(p, dtype=torch.float32).reshape(prev.shape))
            tgt.copy_(torch.as_tensor(t, dtype=torch.float32).reshape(tgt.shape))
            g.replay()

        step.graph, step.inputs = g, (ob, prev, tgt)
        return step

    def final_state(self, windows: int) -> torch.Tensor:
        """final_state_batch [2, B, 200] = (c, h) of the last forward pass over `windows`
        windows (rollout/step: computed with the parameters before that step's update, as
        the reference's sess.run([loss, final_state_batch, minimize_adam]) returns it,
        backup/lstm_bbpt.py:147-155)."""
        out = torch.empty(2, int(windows), NUM_UNITS, dtype=torch.float32, device=self.device)
        self._sync_stream()
        nat.check(self._lib.rdl_final_state(self._h, int(windows), nat.ptr(out)), "rdl_final_state")
        return out

    def grad(self) -> torch.Tensor:
        return self._grad

    def counter(self) -> int:
        v = ctypes.c_int64()
        nat.check(self._lib.rdl_get_counter(self._h, ctypes.byref(v)), "rdl_get_counter")
        return v.value

    def metrics(self, count: int = 1) -> np.ndarray:
        """[count, 4]: loss, sum |mu_s - mu_t|^2, rows (T x B), 0."""
        out = np.zeros((count, 4), np.float64)
        nat.check(self._lib.rdl_read_metrics(self._h, count, out.ctypes.data_as(ctypes.c_void_p)),
                  "rdl_read_metrics")
        return out
