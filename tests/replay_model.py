"""NumPy model of the device replay ring (include/reacher_replay.h): the ring with its three pushes
(wrap-around included), the Philox draw and the gathers.  Not a test: tests/test_replay_host.py checks
the model against itself, tests/test_replay_gpu.py pins the kernels to it bitwise (the feature only
copies floats and draws integers, so no tolerance exists anywhere)."""
import numpy as np

from oracle.refnet_np import philox4x32_10

STEPS, REC = 50, 21
F_REW, F_T, F_S, F_WITH = 11, 12, 16, 20
START_PER_WINDOW, START_COMMON = 0, 1
M32 = (1 << 32) - 1


class RingModel:
    def __init__(self, capacity, seed=0):
        self.capacity, self.seed = int(capacity), int(seed)
        self.ring = np.zeros((self.capacity, STEPS, REC), np.float32)
        self.pushed = 0
        self.draws = 0

    def reset(self):
        self.pushed = self.draws = 0

    def stored(self):
        return min(self.pushed, self.capacity)

    # -- pushes: episode q of a call gets global index pushed + q, slot (pushed + q) % capacity
    def push_episodes(self, rec):
        rec = np.asarray(rec, np.float32).reshape(-1, STEPS, REC)
        assert 1 <= rec.shape[0] <= self.capacity
        for q, ep in enumerate(rec):
            self.ring[(self.pushed + q) % self.capacity] = ep
        self.pushed += rec.shape[0]

    def push_steps(self, records):
        """records [K, n, 21] step-major; episode q = (k // 50) n + i."""
        r = np.asarray(records, np.float32)
        K, n, _ = r.shape
        assert K >= STEPS and K % STEPS == 0 and (K // STEPS) * n <= self.capacity
        # [K/50, 50, n, 21] -> [K/50, n, 50, 21]
        self.push_episodes(r.reshape(K // STEPS, STEPS, n, REC).transpose(0, 2, 1, 3))

    def push_rows(self, x, t_pdflat, s_pdflat, reward, carry=None, stepped_with=1.0):
        """rdm_envs_act's outputs; rew of record (k, i) = reward[k-1, i], carry[i] at k = 0."""
        x, t, rew = np.asarray(x, np.float32), np.asarray(t_pdflat, np.float32), np.asarray(reward, np.float32)
        K, n, _ = x.shape
        s = np.zeros((K, n, 4), np.float32) if s_pdflat is None else np.asarray(s_pdflat, np.float32)
        r = np.zeros((K, n, REC), np.float32)
        r[..., :11] = x[..., :11]
        r[1:, :, F_REW] = rew[:-1]
        r[0, :, F_REW] = 0.0 if carry is None else np.asarray(carry, np.float32)
        r[..., F_T:F_S] = t
        r[..., F_S:F_WITH] = s
        r[..., F_WITH] = np.float32(stepped_with)
        self.push_steps(r)

    # -- the draw of one sample launch (does not advance `draws`)
    def draw(self, B, span, recent=0, window_base=0, common=False):
        """(slot [B], start [B]) for the current counters; span = 51 - T (windows) or 50 (rows)."""
        d = self.draws & M32
        k0, k1 = self.seed & M32, (self.seed >> 32) & M32
        w = int(window_base) + np.arange(int(B), dtype=np.uint64)
        z = np.zeros(int(B), np.uint64)
        o = philox4x32_10([w & np.uint64(M32), w >> np.uint64(32), z + np.uint64(d), z], k0, k1).astype(np.uint64)
        count = self.stored()
        if recent > 0:
            count = min(count, int(recent))
        rank = (o[0] * np.uint64(count)) >> np.uint64(32)
        slot = (np.uint64(self.pushed - count) + rank) % np.uint64(self.capacity)
        sw = o[1]
        if common:
            c = philox4x32_10([[M32], [M32], [d], [1]], k0, k1).astype(np.uint64)
            sw = np.broadcast_to(c[0], (int(B),))
        start = (sw * np.uint64(span)) >> np.uint64(32)
        return slot.astype(np.int64), start.astype(np.int64)

    def _prev(self):
        """[capacity, 50, 5]: t_pdflat | rew of the previous record of the same episode, zeros at 0."""
        prev = np.zeros((self.capacity, STEPS, 5), np.float32)
        prev[:, 1:, :4] = self.ring[:, :-1, F_T:F_S]
        prev[:, 1:, 4] = self.ring[:, :-1, F_REW]
        return prev

    def sample_windows(self, T, B, start_mode=START_PER_WINDOW, recent=0, window_base=0):
        """(ob_w [T,B,11], prev_w [T,B,4], t_w [T,B,4], prew_w [T,B,1], idx [B,2] int32); draws += 1."""
        slot, start = self.draw(B, STEPS + 1 - T, recent, window_base, start_mode == START_COMMON)
        self.draws += 1
        j = start[None, :] + np.arange(T)[:, None]                   # [T, B]
        rec, prev = self.ring[slot[None, :], j], self._prev()[slot[None, :], j]
        idx = np.stack([slot, start], 1).astype(np.int32)
        return (rec[..., :11].copy(), prev[..., :4].copy(), rec[..., F_T:F_S].copy(), prev[..., 4:].copy(), idx)

    def sample_rows(self, B, recent=0, window_base=0):
        """(x [B,16], t_pdflat [B,4], idx [B,2] int32 = slot, step); draws += 1."""
        slot, step = self.draw(B, STEPS, recent, window_base, False)
        self.draws += 1
        rec, prev = self.ring[slot, step], self._prev()[slot, step]
        x = np.concatenate([rec[:, :11], prev], 1)
        return x, rec[:, F_T:F_S].copy(), np.stack([slot, step], 1).astype(np.int32)
