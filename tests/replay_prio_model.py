"""NumPy / Python-integer model of the prioritised replay draw (include/reacher_replay_priority.h): the
uint32 table beside tests.replay_model.RingModel's ring, the read clamp, the float32 score and its
quantisation, what a push writes, the maximum-over-writers update with its skipped indices, and the
draw.  Not a test: tests/test_replay_prio_host.py checks the model against itself and against the
weights, tests/test_replay_prio_gpu.py pins the kernels to it bitwise (the score is four float32
operations with one rounding each, everything else is integer, so no tolerance exists anywhere)."""
from bisect import bisect_right

import numpy as np

from oracle.refnet_np import philox4x32_10
from tests.replay_model import F_S, F_T, REC, STEPS, RingModel

PRIO_MAX = 1 << 24
SQERR, ERR = 0, 1
INIT_CONST, INIT_RECORD = 0, 1
M32 = (1 << 32) - 1
f32 = np.float32


def clamp(q):
    """what every read of an entry returns: 1 .. 2^24"""
    return np.clip(np.asarray(q, np.uint32).astype(np.int64), 1, PRIO_MAX)


def quantise(S, t, measure, shift, q_min):
    """uint32 entries for outputs S [..., >= 2] against teacher outputs t [..., >= 2] (the two means):
    e = S - t; d = e0 e0 + e1 e1 (each product and the sum rounded to float32); sqrt for ERR;
    v = score 2^shift; 2^24 unless v < 2^24 (NaN, inf), else trunc(v); floored at q_min."""
    S, t = np.asarray(S, f32), np.asarray(t, f32)
    with np.errstate(all="ignore"):
        e0, e1 = (S[..., 0] - t[..., 0]).astype(f32), (S[..., 1] - t[..., 1]).astype(f32)
        d = ((e0 * e0).astype(f32) + (e1 * e1).astype(f32)).astype(f32)
        score = np.sqrt(d).astype(f32) if measure == ERR else d
        v = (score * f32(2.0 ** shift)).astype(f32)
        small = v < f32(16777216.0)                       # False for NaN and inf
        q = np.where(small, np.where(small, v, f32(0)).astype(np.int64), PRIO_MAX)
    return np.maximum(q, int(q_min)).astype(np.uint32)


class PrioRingModel(RingModel):
    def __init__(self, capacity, seed=0, measure=SQERR, shift=16, q_min=1, q_init=PRIO_MAX, init=INIT_CONST):
        super().__init__(capacity, seed)
        self.measure, self.shift, self.q_min, self.q_init, self.init = measure, shift, q_min, q_init, init
        self.q = np.full((self.capacity, STEPS), q_init, np.uint32)

    # -- pushes: the ring's copy, then the pushed slots' entries --------------------------------
    def push_episodes(self, rec):
        first = self.pushed
        super().push_episodes(rec)           # push_steps and push_rows come through here too
        for g in range(first, self.pushed):
            slot = g % self.capacity
            if self.init == INIT_RECORD:
                ep = self.ring[slot]
                self.q[slot] = quantise(ep[:, F_S:F_S + 4], ep[:, F_T:F_T + 4], self.measure, self.shift, self.q_min)
            else:
                self.q[slot] = self.q_init

    def fill(self, q):
        self.q[:] = q

    # -- updates: every named record ends with the maximum over its writers ----------------------
    def update(self, idx, s_pdflat):
        """idx [B, 2] (slot, start); s_pdflat [B, 4] (rows, T = 1) or [T, B, 4]."""
        s = np.asarray(s_pdflat, f32)
        s = s[None] if s.ndim == 2 else s
        T, best = s.shape[0], {}
        for b, (slot, start) in enumerate(np.asarray(idx, np.int64)):
            if not 0 <= slot < self.capacity or start < 0 or start + T > STEPS:
                continue                                         # skipped on the device
            for p in range(T):
                at = (int(slot), int(start) + p)
                v = int(quantise(s[p, b], self.ring[at][F_T:F_T + 4], self.measure, self.shift, self.q_min))
                best[at] = max(best.get(at, 0), v)
        for at, v in best.items():
            self.q[at] = v

    # -- the draw of one prioritised sample (does not advance `draws`) ---------------------------
    def eligible(self, recent=0):
        """slots of the eligible episodes, rank 0 (the oldest) first"""
        count = self.stored()
        if recent > 0:
            count = min(count, int(recent))
        return [(self.pushed - count + j) % self.capacity for j in range(count)]

    def window_weights(self, T, recent=0):
        """W [count][51 - T] as Python integers: W(slot_j, s) = the sum of the T clamped entries from s"""
        c = clamp(self.q)[self.eligible(recent)].reshape(-1, STEPS)               # int64: sums stay below 2^30
        cs = np.concatenate([np.zeros((len(c), 1), np.int64), np.cumsum(c, 1)], 1)
        return (cs[:, T:] - cs[:, :STEPS + 1 - T]).tolist()

    def draw_prio(self, T, B, recent=0, window_base=0):
        """(slot [B], start [B], prob [B] float32) for the current counters."""
        slots, W = self.eligible(recent), self.window_weights(T, recent)
        X = [0]
        for row in W:
            X.append(X[-1] + sum(row))                           # X_j: the exclusive prefix of E
        total = X[-1]
        d = self.draws & M32
        w = int(window_base) + np.arange(int(B), dtype=np.uint64)
        z = np.zeros(int(B), np.uint64)
        o = philox4x32_10([w & np.uint64(M32), w >> np.uint64(32), z + np.uint64(d), z + np.uint64(2)],
                          self.seed & M32, (self.seed >> 32) & M32)
        slot, start, prob = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, f32)
        for b in range(int(B)):
            target = (((int(o[0][b]) << 32) | int(o[1][b])) * total) >> 64
            rank = bisect_right(X, target) - 1                   # X_rank <= target < X_{rank + 1}
            rem, run = target - X[rank], 0
            for s, wgt in enumerate(W[rank]):
                run += wgt
                if run > rem:
                    break
            slot[b], start[b] = slots[rank], s
            prob[b] = f32(np.float64(W[rank][s]) / np.float64(total))
        return slot, start, prob

    def sample_windows_prio(self, T, B, recent=0, window_base=0):
        """(ob_w, prev_w, t_w, prew_w, idx [B, 2] int32, prob [B] f32); draws += 1."""
        slot, start, prob = self.draw_prio(T, B, recent, window_base)
        self.draws += 1
        j = start[None, :] + np.arange(T)[:, None]
        rec, prev = self.ring[slot[None, :], j], self._prev()[slot[None, :], j]
        idx = np.stack([slot, start], 1).astype(np.int32)
        return (rec[..., :11].copy(), prev[..., :4].copy(), rec[..., F_T:F_S].copy(), prev[..., 4:].copy(), idx, prob)

    def sample_rows_prio(self, B, recent=0, window_base=0):
        """(x [B, 16], t_pdflat [B, 4], idx [B, 2] int32 = slot, step, prob [B] f32); draws += 1."""
        slot, step, prob = self.draw_prio(1, B, recent, window_base)
        self.draws += 1
        rec, prev = self.ring[slot, step], self._prev()[slot, step]
        return (np.concatenate([rec[:, :11], prev], 1), rec[:, F_T:F_S].copy(),
                np.stack([slot, step], 1).astype(np.int32), prob)


assert REC == 21
