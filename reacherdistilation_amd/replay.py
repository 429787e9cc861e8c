"""Host layer of the device-resident episode replay ring (include/reacher_replay.h).

``ReplayRing`` keeps whole 50-step episodes on the device in the dataset's record layout and draws
training batches of any size from them with a kernel: the aggregate half of the reference's DAgger
loop (dataset.py:166-194) for the batched paths.  Pushes take what the envs and evaluation calls
write (``push_steps``: StudentLstmTrainer.act_envs / step_envs records; ``push_episodes``:
evaluate / collect_episodes / collect_reward records; ``push_rows``: a StudentMlpTrainer.act_envs
result); ``sample_windows`` / ``sample_rows`` return what StudentLstmTrainer.step /
StudentMlpTrainer.step take.  The episode and draw counters live on the device, so nothing here
waits on the GPU, no index tensor is built on the host, and a ``torch.cuda.graph`` holding push,
sample and step replays the NEXT push and the NEXT draw.  Output buffers are allocated once per
(T, B) and reused: clone a result to keep it past the next sample of the same shape.

Prioritised draws (include/reacher_replay_priority.h): ``enable_priorities`` puts a uint32 priority per
record beside the ring (``ring.priorities``), the pushes fill it, ``update_priorities`` refreshes it from
the student's outputs on a sampled batch, and ``sample_rows`` / ``sample_windows`` with
``prioritized=True`` draw a window with probability (sum of its records' priorities) / total, still
with no host RNG, no index upload and no sync.  A ring that never enables them launches what it did.

Single GPU: one ring per process (``window_base`` lets ranks draw disjoint streams).
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as nat
from .config import EPISODE_STEPS, OBSPACE_SHAPE, PDFLAT_SHAPE

P = nat.P
I32, I64, U64, F32, INT = nat.I32, nat.I64, nat.U64, nat.F32, nat.INT
U32 = ctypes.c_uint32

REC = 21                                   # ob[11] | rew | t_pdflat[4] | s_pdflat[4] | stepped_with
ROW = OBSPACE_SHAPE + PDFLAT_SHAPE + 1     # the reference MLP student's input row
START_PER_WINDOW, START_COMMON = 0, 1      # RD_REPLAY_START_*
MAX_BATCH = 1 << 22                        # RD_REPLAY_MAX_BATCH
PRIO_MAX = 1 << 24                         # RD_REPLAY_PRIO_MAX: the largest priority a read returns
PRIO_MAX_CAPACITY = 1 << 22                # RD_REPLAY_PRIO_MAX_CAPACITY
PRIO_SCAN_TILE = 256                       # RD_REPLAY_PRIO_SCAN_TILE: episodes per workgroup of the scan
PRIO_SQERR, PRIO_ERR = 0, 1                # RD_PRIO_*: the score's measure
PRIO_INIT_CONST, PRIO_INIT_RECORD = 0, 1   # RD_PRIO_INIT_*: what a push writes
_MEASURES = {"sqerr": PRIO_SQERR, "err": PRIO_ERR}
_INITS = {"const": PRIO_INIT_CONST, "record": PRIO_INIT_RECORD}


class RdReplayConfig(ctypes.Structure):
    _fields_ = [("capacity", I64), ("max_batch", I64)]


class RdReplaySample(ctypes.Structure):
    _fields_ = [("steps", I32), ("start_mode", I32), ("windows", I64), ("window_base", I64), ("recent", I64),
                ("seed", U64)]


class RdReplayPrioConfig(ctypes.Structure):
    _fields_ = [("measure", I32), ("shift", I32), ("q_min", U32), ("q_init", U32), ("init_mode", I32),
                ("reserved", I32)]


nat.register({
    "rd_replay_prio_enable": (INT, [P, ctypes.POINTER(RdReplayPrioConfig), P]),
    "rd_replay_prio_configure": (INT, [P, ctypes.POINTER(RdReplayPrioConfig)]),
    "rd_replay_prio_enabled": (INT, [P]),
    "rd_replay_prio_table": (P, [P]),
    "rd_replay_prio_fill": (INT, [P, U32]),
    "rd_replay_prio_update_rows": (INT, [P, P, P, I64]),
    "rd_replay_prio_update_windows": (INT, [P, P, P, I32, I64]),
    "rd_replay_prio_sample_rows": (INT, [P, ctypes.POINTER(RdReplaySample), P, P, P, P]),
    "rd_replay_prio_sample_windows": (INT, [P, ctypes.POINTER(RdReplaySample), P, P, P, P, P, P]),
})

nat.register({
    "rd_replay_create": (INT, [ctypes.POINTER(P), ctypes.POINTER(RdReplayConfig), P, INT, P]),
    "rd_replay_destroy": (INT, [P]),
    "rd_replay_set_stream": (INT, [P, P]),
    "rd_replay_reset": (INT, [P]),
    "rd_replay_ring": (P, [P]),
    "rd_replay_counters": (INT, [P, ctypes.POINTER(I64), ctypes.POINTER(I64)]),
    "rd_replay_push_steps": (INT, [P, P, I64, I64]),
    "rd_replay_push_episodes": (INT, [P, P, I64]),
    "rd_replay_push_rows": (INT, [P, P, P, P, P, P, I64, I64, F32]),
    "rd_replay_push_rows_flags": (INT, [P, P, P, P, P, P, I64, I64, P]),
    "rd_replay_sample_windows": (INT, [P, ctypes.POINTER(RdReplaySample), P, P, P, P, P]),
    "rd_replay_sample_rows": (INT, [P, ctypes.POINTER(RdReplaySample), P, P, P]),
})


class ReplayRing:
    def __init__(self, capacity: int, device="cuda:0", seed: int = 0, max_batch: int = 16384):
        self.capacity, self.max_batch, self.seed = int(capacity), int(max_batch), int(seed)
        if self.capacity < 1 or not 1 <= self.max_batch <= MAX_BATCH:
            raise ValueError(f"capacity >= 1 and 1 <= max_batch <= {MAX_BATCH}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ReplayRing lives on a GPU (HIP) device only; there is no CPU path")
        self._lib = nat.load()
        self.records = torch.zeros(self.capacity, EPISODE_STEPS, REC, dtype=torch.float32, device=self.device)
        c = RdReplayConfig(capacity=self.capacity, max_batch=self.max_batch)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rd_replay_create(ctypes.byref(h), ctypes.byref(c), nat.ptr(self.records),
                                                 self.device.index or 0, nat.stream_handle(self.device)),
                      "rd_replay_create")
        self._h = h
        self._carry = None    # push_rows: the last reward row of the previous call
        self._windows = {}    # (T, B) -> output buffers of sample_windows
        self._rows = {}       # B -> output buffers of sample_rows
        self._probs = {}      # B -> prob [B] of the prioritised samples
        self.priorities = None   # [capacity, 50] int32 (the table's uint32 bits) once enable_priorities ran
        self.last_idx = None     # the idx tensor of the latest sample that asked for one (with_idx)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rd_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync_stream(self):
        nat.check(self._lib.rd_replay_set_stream(self._h, nat.stream_handle(self.device)), "rd_replay_set_stream")

    def _f32(self, t):
        return torch.as_tensor(t, dtype=torch.float32, device=self.device).contiguous()

    # -- pushes ------------------------------------------------------------------------
    def push_steps(self, records):
        """records [K, n, 21], step-major (StudentLstmTrainer.act_envs / step_envs), K a multiple of 50
        and row 0 an episode's step 0: (K / 50) n episodes, at most ``capacity``."""
        r = self._f32(records)
        if r.dim() != 3 or r.shape[2] != REC:
            raise ValueError(f"expected [K, n, {REC}], got {tuple(r.shape)}")
        self._sync_stream()
        nat.check(self._lib.rd_replay_push_steps(self._h, nat.ptr(r), r.shape[0], r.shape[1]), "rd_replay_push_steps")
        self._keep = r

    def push_episodes(self, rec):
        """rec [..., 50, 21], episode-major (evaluate(records=True).records, evaluate.collect_episodes,
        teacher.collect_reward): every leading index is one episode, pushed in flattened order."""
        r = self._f32(rec)
        if r.dim() < 2 or tuple(r.shape[-2:]) != (EPISODE_STEPS, REC):
            raise ValueError(f"expected [..., {EPISODE_STEPS}, {REC}], got {tuple(r.shape)}")
        r = r.reshape(-1, EPISODE_STEPS, REC)
        self._sync_stream()
        nat.check(self._lib.rd_replay_push_episodes(self._h, nat.ptr(r), r.shape[0]), "rd_replay_push_episodes")
        self._keep = r

    def push_rows(self, r, stepped_with=None):
        """r: a StudentMlpTrainer.act_envs / step_envs result (x [K, n, 16], t_pdflat, s_pdflat, reward
        [K, n]), K a multiple of 50 from an episode's step 0.  The records' rew field is the reward the
        env's previous step returned; the ring keeps ``r.reward[-1]`` as the next call's carry (zeros
        before the first call and after reset_carry()).  ``stepped_with``: the records' last field, one
        float for every record (default 1: the student stepped) or a [K, n] tensor with a value per
        record (StudentMlpTrainer.stepped_with after a call under a teacher share;
        rd_replay_push_rows_flags)."""
        x, t, s, rew = self._f32(r.x), self._f32(r.t_pdflat), self._f32(r.s_pdflat), self._f32(r.reward)
        if x.dim() != 3 or x.shape[2] != ROW or tuple(rew.shape) != tuple(x.shape[:2]) or \
                tuple(t.shape) != (*x.shape[:2], PDFLAT_SHAPE) or tuple(s.shape) != tuple(t.shape):
            raise ValueError("expected x [K, n, 16], t_pdflat and s_pdflat [K, n, 4], reward [K, n]")
        K, n = x.shape[:2]
        if self._carry is None or self._carry.shape[0] != n:
            self._carry = torch.zeros(n, dtype=torch.float32, device=self.device)
        flags = None
        if torch.is_tensor(stepped_with):
            flags = self._f32(stepped_with)
            if tuple(flags.shape) != (K, n):
                raise ValueError(f"a stepped_with tensor must be [K, n] = [{K}, {n}], got {tuple(flags.shape)}")
        self._sync_stream()
        if flags is not None:
            nat.check(self._lib.rd_replay_push_rows_flags(self._h, nat.ptr(x), nat.ptr(t), nat.ptr(s), nat.ptr(rew),
                                                          nat.ptr(self._carry), K, n, nat.ptr(flags)),
                      "rd_replay_push_rows_flags")
        else:
            nat.check(self._lib.rd_replay_push_rows(self._h, nat.ptr(x), nat.ptr(t), nat.ptr(s), nat.ptr(rew),
                                                    nat.ptr(self._carry), K, n,
                                                    1.0 if stepped_with is None else float(stepped_with)),
                      "rd_replay_push_rows")
        self._carry.copy_(rew[K - 1])   # behind the push on the stream
        self._keep = (x, t, s, rew, flags)

    def reset_carry(self):
        """The next push_rows starts from a zero carried reward (after the envs were reset)."""
        if self._carry is not None:
            self._carry.zero_()

    # -- draws -------------------------------------------------------------------------
    def _sample(self, T, B, common_start, recent, window_base):
        B = int(B)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"B must be 1 .. max_batch = {self.max_batch}, got {B}")
        return RdReplaySample(steps=int(T), start_mode=START_COMMON if common_start else START_PER_WINDOW, windows=B,
                              window_base=int(window_base), recent=int(recent), seed=self.seed % 2 ** 64)

    def _prob(self, B):
        if B not in self._probs:
            self._probs[B] = torch.zeros(B, dtype=torch.float32, device=self.device)
        return self._probs[B]

    def _need_priorities(self):
        if self.priorities is None:
            raise ValueError("priorities are not enabled: call enable_priorities() first")

    def sample_windows(self, T: int, B: int, common_start: bool = False, recent: int = 0, window_base: int = 0,
                       with_idx: bool = False, prioritized: bool = False, with_prob: bool = False):
        """B windows of T consecutive records drawn on the device: (ob_w [T, B, 11], prev_w [T, B, 4],
        t_w [T, B, 4], prew_w [T, B, 1][, idx [B, 2] int32 = slot, start]), the operands of
        StudentLstmTrainer.step(ob_w, prev_w, t_w).  Episodes uniform over the stored ones (the newest
        ``recent`` if > 0), starts uniform over 0 .. 50 - T per window, or one per batch
        (``common_start``, the reference's training_batches).  The tensors are the ring's own per (T, B).
        ``prioritized``: a window is drawn with probability (sum of its T records' priorities) / (that of
        all eligible windows) instead (enable_priorities first; no common start); ``with_prob`` appends
        that probability, prob [B] f32."""
        if (prioritized or with_prob) and (common_start or not prioritized):
            raise ValueError("with_prob needs prioritized=True, and a prioritised draw has no common start")
        if prioritized:
            self._need_priorities()
        s = self._sample(T, B, common_start, recent, window_base)
        T, B = s.steps, s.windows
        if (T, B) not in self._windows:
            kw = dict(dtype=torch.float32, device=self.device)
            self._windows[T, B] = (torch.zeros(T, B, OBSPACE_SHAPE, **kw), torch.zeros(T, B, PDFLAT_SHAPE, **kw),
                                   torch.zeros(T, B, PDFLAT_SHAPE, **kw), torch.zeros(T, B, 1, **kw),
                                   torch.zeros(B, 2, dtype=torch.int32, device=self.device))
        ob_w, prev_w, t_w, prew_w, idx = self._windows[T, B]
        if with_idx:
            self.last_idx = idx
        self._sync_stream()
        if prioritized:
            prob = self._prob(B) if with_prob else None
            nat.check(self._lib.rd_replay_prio_sample_windows(
                self._h, ctypes.byref(s), nat.ptr(ob_w), nat.ptr(prev_w), nat.ptr(t_w), nat.ptr(prew_w),
                nat.ptr(idx) if with_idx else None, nat.ptr(prob) if with_prob else None), "rd_replay_prio_sample_windows")
            return (ob_w, prev_w, t_w, prew_w) + ((idx,) if with_idx else ()) + ((prob,) if with_prob else ())
        nat.check(self._lib.rd_replay_sample_windows(self._h, ctypes.byref(s), nat.ptr(ob_w), nat.ptr(prev_w),
                                                     nat.ptr(t_w), nat.ptr(prew_w), nat.ptr(idx) if with_idx else None),
                  "rd_replay_sample_windows")
        return (ob_w, prev_w, t_w, prew_w, idx) if with_idx else (ob_w, prev_w, t_w, prew_w)

    def sample_rows(self, B: int, recent: int = 0, window_base: int = 0, with_idx: bool = False,
                    prioritized: bool = False, with_prob: bool = False):
        """B single records drawn on the device as (x [B, 16], t_pdflat [B, 4][, idx [B, 2] int32 = slot,
        step]), the operands of StudentMlpTrainer.step: x = ob | the previous record's t_pdflat | its rew
        (zeros at step 0), exactly the row StudentMlpTrainer.act_envs emitted for that step.
        ``prioritized``: a record is drawn with probability priority / (the eligible records' total)
        instead (enable_priorities first); ``with_prob`` appends that probability, prob [B] f32."""
        if with_prob and not prioritized:
            raise ValueError("with_prob needs prioritized=True")
        if prioritized:
            self._need_priorities()
        s = self._sample(1, B, False, recent, window_base)
        B = s.windows
        if B not in self._rows:
            self._rows[B] = (torch.zeros(B, ROW, dtype=torch.float32, device=self.device),
                             torch.zeros(B, PDFLAT_SHAPE, dtype=torch.float32, device=self.device),
                             torch.zeros(B, 2, dtype=torch.int32, device=self.device))
        x, t, idx = self._rows[B]
        if with_idx:
            self.last_idx = idx
        self._sync_stream()
        if prioritized:
            prob = self._prob(B) if with_prob else None
            nat.check(self._lib.rd_replay_prio_sample_rows(self._h, ctypes.byref(s), nat.ptr(x), nat.ptr(t),
                                                           nat.ptr(idx) if with_idx else None,
                                                           nat.ptr(prob) if with_prob else None),
                      "rd_replay_prio_sample_rows")
            return (x, t) + ((idx,) if with_idx else ()) + ((prob,) if with_prob else ())
        nat.check(self._lib.rd_replay_sample_rows(self._h, ctypes.byref(s), nat.ptr(x), nat.ptr(t),
                                                  nat.ptr(idx) if with_idx else None), "rd_replay_sample_rows")
        return (x, t, idx) if with_idx else (x, t)

    # -- priorities (include/reacher_replay_priority.h) -----------------------------------
    @staticmethod
    def _prio_config(measure, shift, q_min, q_init, init):
        if measure not in _MEASURES or init not in _INITS:
            raise ValueError(f"measure one of {sorted(_MEASURES)}, init one of {sorted(_INITS)}")
        if not 0 <= int(shift) <= 24 or not 1 <= int(q_min) <= PRIO_MAX or not 1 <= int(q_init) <= PRIO_MAX:
            raise ValueError(f"shift 0 .. 24, q_min and q_init 1 .. {PRIO_MAX}")
        return RdReplayPrioConfig(measure=_MEASURES[measure], shift=int(shift), q_min=int(q_min), q_init=int(q_init),
                                  init_mode=_INITS[init], reserved=0)

    def enable_priorities(self, measure: str = "sqerr", shift: int = 16, q_min: int = 1, q_init: int = PRIO_MAX,
                          init: str = "const", table=None):
        """A priority per record, ``ring.priorities`` [capacity, 50] int32 (read as uint32; every read
        clamps to 1 .. 2^24), all ``q_init`` to begin with; once per ring.  A record's score is the
        student's squared error against the teacher's mean over the two action dims ("sqerr") or its root
        ("err"), quantised as max(min(trunc(score 2^shift), 2^24), q_min).  From now on every push writes
        its episodes' entries: ``q_init`` (init="const") or the score of the record's own s_pdflat
        (init="record": the student as it was when it acted).  ``table``: a caller's int32 device tensor
        [capacity, 50] (possibly a view into a larger one) instead of the ring's own.  Any torch op may
        write ``ring.priorities`` between calls (an exponent, a decay)."""
        if self.priorities is not None:
            raise ValueError("priorities are already enabled")
        if self.capacity > PRIO_MAX_CAPACITY:
            raise ValueError(f"priorities need capacity <= {PRIO_MAX_CAPACITY}")
        c = self._prio_config(measure, shift, q_min, q_init, init)
        if table is None:
            table = torch.zeros(self.capacity, EPISODE_STEPS, dtype=torch.int32, device=self.device)
        elif table.dtype != torch.int32 or tuple(table.shape) != (self.capacity, EPISODE_STEPS) or \
                not table.is_contiguous() or table.device != self.records.device:
            raise ValueError(f"table: a contiguous int32 tensor [{self.capacity}, {EPISODE_STEPS}] on {self.device}")
        self._sync_stream()
        with torch.cuda.device(self.device):
            nat.check(self._lib.rd_replay_prio_enable(self._h, ctypes.byref(c), nat.ptr(table)), "rd_replay_prio_enable")
        self.priorities, self._prio = table, c

    def set_priority_init(self, init: str | None = None, *, measure: str | None = None, shift: int | None = None,
                          q_min: int | None = None, q_init: int | None = None):
        """Replace what the pushes write (``init``) and, if given, the other fields of the config, for the
        calls issued from now on (rd_replay_prio_configure: host-only, nothing is launched)."""
        self._need_priorities()
        old = self._prio
        inv_m = {v: k for k, v in _MEASURES.items()}
        inv_i = {v: k for k, v in _INITS.items()}
        c = self._prio_config(inv_m[old.measure] if measure is None else measure,
                              old.shift if shift is None else shift, old.q_min if q_min is None else q_min,
                              old.q_init if q_init is None else q_init, inv_i[old.init_mode] if init is None else init)
        nat.check(self._lib.rd_replay_prio_configure(self._h, ctypes.byref(c)), "rd_replay_prio_configure")
        self._prio = c

    def fill_priorities(self, q: int):
        """Every entry of the table = q (1 .. 2^24)."""
        self._need_priorities()
        if not 1 <= int(q) <= PRIO_MAX:
            raise ValueError(f"q must be 1 .. {PRIO_MAX}")
        self._sync_stream()
        nat.check(self._lib.rd_replay_prio_fill(self._h, int(q)), "rd_replay_prio_fill")

    def update_priorities(self, idx, s_pdflat):
        """The records a sample named get the score of the student's current output on them: ``idx``
        [B, 2] int32 as the sample returned it, ``s_pdflat`` [B, 4] (StudentMlpTrainer.forward on the
        sampled x) or [T, B, 4] (StudentLstmTrainer.forward on the sampled windows).  A record named more
        than once ends with the maximum; entries outside the ring are skipped on the device."""
        self._need_priorities()
        s = self._f32(s_pdflat)
        if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[1] != 2 or not idx.is_contiguous() or \
                idx.device != self.records.device:
            raise ValueError("idx: a contiguous int32 tensor [B, 2] on the ring's device")
        B = idx.shape[0]
        if s.dim() not in (2, 3) or s.shape[-1] != PDFLAT_SHAPE or s.shape[-2] != B or not 1 <= B <= self.max_batch:
            raise ValueError(f"s_pdflat [B, 4] or [T, B, 4] with B = {B} = idx's, 1 .. max_batch")
        self._sync_stream()
        if s.dim() == 2:
            nat.check(self._lib.rd_replay_prio_update_rows(self._h, nat.ptr(idx), nat.ptr(s), B),
                      "rd_replay_prio_update_rows")
        else:
            nat.check(self._lib.rd_replay_prio_update_windows(self._h, nat.ptr(idx), nat.ptr(s), s.shape[0], B),
                      "rd_replay_prio_update_windows")
        self._keep_prio = (idx, s)

    # -- counters ----------------------------------------------------------------------
    def counters(self):
        """(pushed, draws) as the device holds them; waits for the stream."""
        p, d = ctypes.c_int64(), ctypes.c_int64()
        self._sync_stream()
        nat.check(self._lib.rd_replay_counters(self._h, ctypes.byref(p), ctypes.byref(d)), "rd_replay_counters")
        return p.value, d.value

    def stored(self) -> int:
        """Episodes a draw can reach: min(pushed, capacity); waits for the stream."""
        return min(self.counters()[0], self.capacity)

    def reset(self):
        """Both counters to 0 (the ring's floats stay) and the carried reward of push_rows to 0."""
        self._sync_stream()
        nat.check(self._lib.rd_replay_reset(self._h), "rd_replay_reset")
        self.reset_carry()
