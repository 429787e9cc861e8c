"""The sensor faults of the students' closed loop (include/reacher_obs_faults.h) from NumPy:
oracle/refnet_np.philox4x32_10 and the header's definition -- for env e = env_base + i, the record of
step s of Philox episode `episode`, component k = 0..10

    w^q    = Philox4x32-10(ctr = {e lo, e hi, episode, 0x20000000 | (q << 8) | s}, key = seed),  q = k / 4
    u_k    = (w^q[k % 4] >> 8) 2^-24
    keep_k = u_k < keep_prob
    seen_k = keep_k ? (DROPOUT ? ob_k / keep_prob : ob_k) : 0

in float32.  Shared by tests/test_obs_faults_host.py and the *_faults_gpu.py suites, with the seeds and
shapes of the GPU runs, so that the host suite can check the kept fraction over exactly those."""
import numpy as np

from oracle import refnet_np as rn

EPISODE = 50
OB = 11
CLEAN, DROPOUT, MISSING = 0, 1, 2
MODES = {"none": CLEAN, "dropout": DROPOUT, "missing": MISSING}
FAULT_BIT = 0x20000000
KEEP = 0.5   # the GPU suites' keep_prob
# (mask seed, env_base, n_envs, lockstep steps from the attach) of the GPU suites' runs against the
# stepwise loop; the kept fraction is checked over each, and over the largest for every keep_prob
RUNS = [(11, 5, 1, 100), (11, 5, 17, 100), (11, 5, 83, 100)]
# rd_mask_obs against this model: env ids across 2^32, a seed with a high word (tests/action_noise.py's)
WIDE_SEED, WIDE_BASE = 0x9E3779B97F4A7C15, 2 ** 32 - 40


def counters(env_base, n, episode, step, q):
    """the four Philox counter words [4][n] (uint64 holding 32-bit values) of call q = 0, 1, 2"""
    e = np.arange(n, dtype=np.uint64) + np.uint64(env_base)
    return [e & rn.M32, e >> np.uint64(32), np.full(n, episode, np.uint64),
            np.full(n, FAULT_BIT | (int(q) << 8) | int(step), np.uint64)]


def words(seed, env_base, n, episode, step):
    """the 12 Philox words uint32 [n, 12] of envs env_base .. env_base + n - 1 at (episode, step): word k
    decides component k (the twelfth is not used)"""
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    w = [rn.philox4x32_10(counters(env_base, n, episode, step, q), k0, k1) for q in range(3)]
    return np.stack([np.asarray(w[q][j], np.uint32) for q in range(3) for j in range(4)], axis=1)


def kept(seed, env_base, n, episode, step, keep_prob):
    """keep_k bool [n, 11]"""
    u = (words(seed, env_base, n, episode, step)[:, :OB] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(keep_prob)


def kept_table(seed, env_base, n, steps, keep_prob, start=0):
    """keep [steps, n, 11] for lockstep envs from global step `start` (episode g // 50, step g % 50)"""
    return np.stack([kept(seed, env_base, n, g // EPISODE, g % EPISODE, keep_prob) for g in range(start, start + steps)])


def see(ob, keep, mode, keep_prob):
    """seen float32 [n, 11] from ob [n, 11] and keep [n, 11]"""
    f = np.float32
    ob = np.asarray(ob, f)
    if mode == CLEAN:
        return ob.copy()
    scaled = (ob / f(keep_prob)).astype(f) if mode == DROPOUT else ob
    return np.where(keep, scaled, f(0.0)).astype(f)
