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

Single GPU: one ring per process (``window_base`` lets ranks draw disjoint streams).
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as nat
from .config import EPISODE_STEPS, OBSPACE_SHAPE, PDFLAT_SHAPE

P = nat.P
I32, I64, U64, F32, INT = nat.I32, nat.I64, nat.U64, nat.F32, nat.INT

REC = 21                                   # ob[11] | rew | t_pdflat[4] | s_pdflat[4] | stepped_with
ROW = OBSPACE_SHAPE + PDFLAT_SHAPE + 1     # the reference MLP student's input row
START_PER_WINDOW, START_COMMON = 0, 1      # RD_REPLAY_START_*
MAX_BATCH = 1 << 22                        # RD_REPLAY_MAX_BATCH


class RdReplayConfig(ctypes.Structure):
    _fields_ = [("capacity", I64), ("max_batch", I64)]


class RdReplaySample(ctypes.Structure):
    _fields_ = [("steps", I32), ("start_mode", I32), ("windows", I64), ("window_base", I64), ("recent", I64),
                ("seed", U64)]


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

    def sample_windows(self, T: int, B: int, common_start: bool = False, recent: int = 0, window_base: int = 0,
                       with_idx: bool = False):
        """B windows of T consecutive records drawn on the device: (ob_w [T, B, 11], prev_w [T, B, 4],
        t_w [T, B, 4], prew_w [T, B, 1][, idx [B, 2] int32 = slot, start]), the operands of
        StudentLstmTrainer.step(ob_w, prev_w, t_w).  Episodes uniform over the stored ones (the newest
        ``recent`` if > 0), starts uniform over 0 .. 50 - T per window, or one per batch
        (``common_start``, the reference's training_batches).  The tensors are the ring's own per (T, B)."""
        s = self._sample(T, B, common_start, recent, window_base)
        T, B = s.steps, s.windows
        if (T, B) not in self._windows:
            kw = dict(dtype=torch.float32, device=self.device)
            self._windows[T, B] = (torch.zeros(T, B, OBSPACE_SHAPE, **kw), torch.zeros(T, B, PDFLAT_SHAPE, **kw),
                                   torch.zeros(T, B, PDFLAT_SHAPE, **kw), torch.zeros(T, B, 1, **kw),
                                   torch.zeros(B, 2, dtype=torch.int32, device=self.device))
        ob_w, prev_w, t_w, prew_w, idx = self._windows[T, B]
        self._sync_stream()
        nat.check(self._lib.rd_replay_sample_windows(self._h, ctypes.byref(s), nat.ptr(ob_w), nat.ptr(prev_w),
                                                     nat.ptr(t_w), nat.ptr(prew_w), nat.ptr(idx) if with_idx else None),
                  "rd_replay_sample_windows")
        return (ob_w, prev_w, t_w, prew_w, idx) if with_idx else (ob_w, prev_w, t_w, prew_w)

    def sample_rows(self, B: int, recent: int = 0, window_base: int = 0, with_idx: bool = False):
        """B single records drawn on the device as (x [B, 16], t_pdflat [B, 4][, idx [B, 2] int32 = slot,
        step]), the operands of StudentMlpTrainer.step: x = ob | the previous record's t_pdflat | its rew
        (zeros at step 0), exactly the row StudentMlpTrainer.act_envs emitted for that step."""
        s = self._sample(1, B, False, recent, window_base)
        B = s.windows
        if B not in self._rows:
            self._rows[B] = (torch.zeros(B, ROW, dtype=torch.float32, device=self.device),
                             torch.zeros(B, PDFLAT_SHAPE, dtype=torch.float32, device=self.device),
                             torch.zeros(B, 2, dtype=torch.int32, device=self.device))
        x, t, idx = self._rows[B]
        self._sync_stream()
        nat.check(self._lib.rd_replay_sample_rows(self._h, ctypes.byref(s), nat.ptr(x), nat.ptr(t),
                                                  nat.ptr(idx) if with_idx else None), "rd_replay_sample_rows")
        return (x, t, idx) if with_idx else (x, t)

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
